"""A delayed-producer harness for the stream contract ("Stream contract"): every entry point does its work on
the caller's stream, behind whatever that stream holds on entry, and has joined its own helper streams when it returns.

The suite's other GPU tests run on the default stream and read results after a host synchronisation, where a missing wait or
a missing join is invisible.  staged() makes such a break deterministic without provoking anything worse than wrong bits:

  (a) the case runs on the default stream, followed by a device synchronisation: the reference (it also warms code objects,
      helper streams and pools, and its host time is the case's enqueue time);
  (b) every float input is overwritten with a DECOY (finite, inside the range of the good values), a fresh non-default stream
      `s` gets a bounded busy-wait (spin), then the copies that put the good values back, then the case - all enqueued while
      the spin is still running - and every output is cloned on `s`.  Only then does the host synchronise.

Work that did not wait for `s` reads decoys and produces other bits than (a): "entry".  The outputs are cloned a second time
after the device synchronisation; clones taken on `s` that differ from those mean the case returned with work outstanding on
a stream that `s` does not wait for: "exit".  The exit check is probabilistic in what it catches - the unjoined work may
happen to finish before the clone runs, and a recycled block may still hold (a)'s identical bits - but it can never raise a
false alarm: with the joins in place the two clones read the same finished memory.  The entry check is only as good as the
delay: an event recorded behind the spin must still be pending when the case returns on the host ("armed"), else the case
fails as "not armed" unless its table entry declares that the entry point synchronises the host by design.

Streams are multiplexed onto a few hardware queues.  A helper stream that shares its queue with `s` runs behind the spin
whether or not it waits for `s`, which hides a missing wait (never the other way round); every staged() call takes the next
stream of torch's pool, so the suite's cases spread over the queues.  Tests about two streams that must OVERLAP pick their pair
with concurrent_pair().

Integer tables (graph indices, scope, segment offsets, bond maps) are valid from the start and are never staged, and decoys
are finite and in range: no run, correct or broken, indexes out of bounds or meets a NaN storm.

Host-side logic (the delay rule, the exemption cap of the case tables) is importable without a GPU: tests/test_streams_cpu.py."""
import time
from collections import namedtuple

import torch

MIN_DELAY_MS = 20.0      # a delay is never shorter than this ...
MAX_DELAY_MS = 100.0     # ... and no single spin is longer than this
DELAY_FACTOR = 5.0       # times the measured host enqueue time: absorbs host jitter on a shared machine
EXEMPT_ONE_IN = 8        # at most one case in eight of a section may be declared host_sync

# name: unique inside its section; build() -> (inputs, fn): the float tensors to stage IN PLACE and fn(inputs) -> outputs (a
# tensor or any nesting of dict / list / tuple of tensors; None entries are skipped).  host_sync: the entry point blocks the
# host by design (it returns Python numbers) - then `reason` says why, and the armed check does not apply.
Case = namedtuple("Case", "name build host_sync reason", defaults=(False, ""))

Result = namedtuple("Result", "name enqueue_ms delay_ms status ref")


class OrderingViolation(AssertionError):
    """kind: 'entry', 'exit' or 'not armed'"""

    def __init__(self, kind, msg):
        super().__init__(f"[{kind}] {msg}")
        self.kind = kind


# ---------------------------------------------------------------------------------------------- host logic
def delay_ms(enqueue_ms: float) -> float:
    """the spin in front of a case whose reference run took `enqueue_ms` on the host"""
    return min(MAX_DELAY_MS, max(MIN_DELAY_MS, DELAY_FACTOR * float(enqueue_ms)))


def check_table(section: str, cases) -> None:
    """names are unique, every exempt case says why, and at most one case in eight is exempt"""
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), f"section {section}: duplicate case names"
    exempt = [c for c in cases if c.host_sync]
    for c in exempt:
        assert c.reason.strip(), f"section {section}: exempt case {c.name!r} gives no reason"
    for c in cases:
        assert c.host_sync or not c.reason, f"section {section}: {c.name!r} gives a reason but is not exempt"
    assert len(exempt) * EXEMPT_ONE_IN <= len(cases), \
        f"section {section}: {len(exempt)} of {len(cases)} cases exempt (at most one in {EXEMPT_ONE_IN})"


def flatten(out, prefix="out"):
    """[(label, tensor)] of every tensor in a nesting of dict / list / tuple, in a fixed order"""
    if out is None:
        return []
    if torch.is_tensor(out):
        return [(prefix, out)]
    if isinstance(out, dict):
        return [x for k in out for x in flatten(out[k], f"{prefix}.{k}")]
    if isinstance(out, (list, tuple)):
        return [x for i, v in enumerate(out) for x in flatten(v, f"{prefix}[{i}]")]
    raise TypeError(f"{prefix}: {type(out).__name__} is neither a tensor nor a nesting of tensors")


def decoy_of(good: torch.Tensor) -> torch.Tensor:
    """Another finite tensor of the same shape: the values shifted by one row (one position for a vector or a single row) and
    pulled a quarter of the way towards their mean - a convex combination inside [min, max] of `good`, column by column for a
    matrix, so a variance column stays positive and a probability stays in [0, 1].  A one-element tensor is halved.  A
    constant tensor has no decoy: the case must not stage one."""
    g = good.detach()
    if g.numel() == 1:
        d = g * 0.5
    elif g.dim() >= 2 and g.shape[0] > 1:
        d = 0.75 * torch.roll(g, 1, dims=0) + 0.25 * g.mean(dim=0, keepdim=True)
    else:
        flat = g.reshape(-1)
        d = 0.75 * torch.roll(flat, 1) + 0.25 * flat.mean()
    d = d.to(good.dtype).reshape(good.shape)
    assert bool(torch.isfinite(d).all()) and not torch.equal(d, good.detach()), "an input without a decoy (constant tensor?)"
    return d


# ---------------------------------------------------------------------------------------------- the delay
_CYCLES_PER_MS = None


def cycles_per_ms() -> float:
    """torch.cuda._sleep cycles per millisecond on this device, measured once per process with two events"""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        torch.cuda._sleep(1000)                                     # (load the kernel outside the measurement)
        torch.cuda.synchronize()
        n = 1_000_000
        for _ in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 2.0:
                break
            n *= 8
        _CYCLES_PER_MS = n / max(ms, 1e-3)
    return _CYCLES_PER_MS


def spin(stream, ms: float) -> None:
    """a bounded busy-wait of `ms` milliseconds (at most MAX_DELAY_MS) enqueued on `stream`"""
    assert 0.0 < ms <= MAX_DELAY_MS, ms
    cycles = int(cycles_per_ms() * ms)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)


def concurrent_pair(work, candidates: int = 6, log=None):
    """Two streams (A, B) of which B demonstrably runs while A is held up: `work()` issued under B completes while a spin on A is
    still pending.  Streams are multiplexed onto a few hardware queues, and two streams that share a queue run one after the
    other - a test of what happens when they OVERLAP has to pick a pair that does.  `work` should enqueue what the test will
    run on B (it may use the library's own helper streams: they must not queue up behind A either)."""
    cands = [torch.cuda.Stream() for _ in range(candidates)]
    probes = 0
    for a in cands:
        for b in cands:
            if a is b:
                continue
            probes += 1
            spin(a, MIN_DELAY_MS)
            ea, eb = torch.cuda.Event(), torch.cuda.Event()
            ea.record(a)
            with torch.cuda.stream(b):
                work()
                eb.record(b)
            eb.synchronize()
            overlapped = not ea.query()
            torch.cuda.synchronize()
            if overlapped:
                if log is not None:
                    log(f"concurrent stream pair found at probe {probes}")
                return a, b
    raise AssertionError(f"no pair among {candidates} streams overlaps: every probe of B waited for the spin on A")


# ---------------------------------------------------------------------------------------------- the staged run
def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit for bit, so a NaN an entry point returns by design (a rank correlation of a constant key) equals itself"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _clones(out):
    return [(k, t.detach().clone()) for k, t in flatten(out)]


def _put(inputs, values):
    with torch.no_grad():
        for t, v in zip(inputs, values):
            t.copy_(v)


def staged(case: Case, log=None, stream=None) -> Result:
    """Run `case` as the module docstring says; raises OrderingViolation, returns the Result (ref: the reference outputs as
    [(label, tensor)]).  `stream`: the caller's stream of run (b), a fresh one by default."""
    inputs, fn = case.build()
    inputs = list(inputs)
    good = [t.detach().clone() for t in inputs]
    decoys = [decoy_of(g) for g in good]
    torch.cuda.synchronize()
    # (a) the reference, on the default stream
    t0 = time.perf_counter()
    out = fn(inputs)
    enqueue = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    ref = _clones(out)
    del out
    assert ref, f"{case.name}: the case returns no tensor"
    # (b) decoys in place, then spin -> good values -> the case, all on s
    _put(inputs, decoys)
    torch.cuda.synchronize()
    D = delay_ms(enqueue)
    s = torch.cuda.Stream() if stream is None else stream
    spin(s, D)
    with torch.cuda.stream(s):
        behind_spin = torch.cuda.Event()
        behind_spin.record(s)
        _put(inputs, good)
        out = fn(inputs)
        armed = not behind_spin.query()                            # the delay outlived the enqueue
        on_s = _clones(out)
    torch.cuda.synchronize()
    after = _clones(out)
    _put(inputs, good)                                             # (a case may update its inputs in place: leave them as given)
    torch.cuda.synchronize()
    status = "armed" if armed else ("exempt" if case.host_sync else "not armed")
    if log is not None:
        log(f"{case.name}: enqueue {enqueue:.3f} ms, delay {D:.0f} ms, {status}"
            + (f" ({case.reason})" if status == "exempt" else ""))
    assert [k for k, _ in on_s] == [k for k, _ in ref], f"{case.name}: the two runs return different structures"
    for (k, a), (_, b) in zip(on_s, after):
        if not same_bits(a, b):
            raise OrderingViolation("exit", f"{case.name}: {k} was still being written when the call returned "
                                            "(clone on the caller's stream != clone after the device synchronisation)")
    for (k, a), (_, r) in zip(on_s, ref):
        if not same_bits(a, r):
            raise OrderingViolation("entry", f"{case.name}: {k} differs from the default-stream run "
                                             "(work that did not wait for the caller's stream read the decoys)")
    if status == "not armed":
        raise OrderingViolation("not armed", f"{case.name}: the {D:.0f} ms delay had ended when the call returned "
                                             "(the entry point blocked the host, or the enqueue took longer)")
    return Result(case.name, enqueue, D, status, ref)
