"""Poisoned allocation: hold the library to "every word read from a caller buffer is written earlier in the same call".

Every wrapper of reactranker_amd hands the library memory it has not initialised (torch.empty / torch.empty_like /
Tensor.new_empty for outputs and scratch, functions._WorkspacePool.take for the step plans' workspace).  A test process mostly
gets such memory as zeros, on which a slab that is summed but never written, a pad column a wide load reads or a partial past
the last block all give right answers.  `poisoned(byte)` makes that memory hold a chosen pattern instead:

    fill   f32               f64               what it catches
    0x00   0                 0                 the control
    0x7F   3.39e38 (finite)  1.4e306 (finite)  a stale word that is ADDED
    0xFF   NaN               NaN               a stale word that is MULTIPLIED by a zero

Integer allocations (int8 ... int64) never hold a byte pattern - a poisoned integer could become an address: they are filled
with the values 0 (fill 0x00) and 1 (both non-zero fills).  bool gets False / True, everything else the byte itself.
torch.zeros* stay as they are: the ticket counters, the Adam moments and the data-parallel bucket are zero by contract.

`fill_dependence(fn)` is the comparison: fn() plain, then under the three fills, everything it returns compared as raw bits.
Nothing is installed at import; `poisoned` restores every name it replaced on exit, also when its body raises."""
import contextlib

import numpy as np
import torch

FILLS = (0x00, 0x7F, 0xFF)
_INDEX_TYPES = (torch.int8, torch.int16, torch.int32, torch.int64)


class Counters:
    def __init__(self):
        self.buffers = 0
        self.bytes = 0
        self.takes = 0           # of the buffers, how many came through _WorkspacePool.take

    def __repr__(self):
        return f"{self.buffers} buffers, {self.bytes} bytes"


def _storage_bytes(orig_empty, t):
    """uint8 view of the whole storage behind `t` (a freshly allocated tensor owns all of it)"""
    st = t.untyped_storage()
    return orig_empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (st.nbytes(),))


def _kept(spare, n):
    """spare as sorted, merged [lo, hi) ranges clamped to [0, n)"""
    out = []
    for lo, hi in sorted((max(0, int(lo)), min(n, int(hi))) for lo, hi in spare):
        if hi <= lo:
            continue
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def fill(orig_empty, t, byte, spare=()):
    """Overwrite every byte of t's storage with the pattern for its dtype (see the module docstring) -> bytes written.
    spare: [lo, hi) byte ranges of the storage to leave as they are (they may overlap or reach past the storage); of an integer
    tensor only the elements that lie wholly outside them are written."""
    n = t.untyped_storage().nbytes()
    if n == 0:
        return 0
    raw = _storage_bytes(orig_empty, t)
    index = t.dtype in _INDEX_TYPES
    es = t.element_size() if index else 1
    value = (0 if byte == 0 else 1) if index else ((1 if byte else 0) if t.dtype == torch.bool else byte)
    written, at = 0, 0
    for lo, hi in _kept(spare, n) + [[n, n]]:
        a, b = (at + es - 1) // es * es, lo // es * es                # whole elements inside the gap [at, lo)
        if b > a:
            (raw[a:b].view(t.dtype) if index else raw[a:b]).fill_(value)
            written += b - a
        at = hi
    return written


@contextlib.contextmanager
def poisoned(byte, spare_pool=()):
    """Replace torch.empty, torch.empty_like, torch.Tensor.new_empty and functions._WorkspacePool.take for the duration:
    each calls the original with unchanged arguments and then fills the new storage with `byte`'s pattern (calls with out=
    and anything that does not return a tensor pass through).  The pool's buffer is refilled on EVERY take, headroom included,
    new or reused; spare_pool lists byte ranges of it to leave alone.  Yields the Counters."""
    assert 0 <= int(byte) <= 0xFF
    from reactranker_amd import functions as Fn
    c = Counters()
    o_empty, o_like, o_new = torch.empty, torch.empty_like, torch.Tensor.new_empty
    o_take = Fn._WorkspacePool.__dict__["take"]                     # the classmethod object itself

    def _done(t, spare=()):
        if isinstance(t, torch.Tensor):
            c.bytes += fill(o_empty, t, byte, spare)
            c.buffers += 1
        return t

    in_take = []

    def empty(*a, **kw):
        return o_empty(*a, **kw) if (kw.get("out") is not None or in_take) else _done(o_empty(*a, **kw))

    def empty_like(*a, **kw):
        return _done(o_like(*a, **kw))

    def new_empty(self, *a, **kw):
        return _done(o_new(self, *a, **kw))

    def take(cls, nbytes, device):
        in_take.append(1)                                           # its own torch.empty is filled here, once, sparing spare_pool
        try:
            t = o_take.__func__(cls, nbytes, device)
        finally:
            in_take.pop()
        c.takes += 1
        return _done(t, spare_pool)

    torch.empty, torch.empty_like, torch.Tensor.new_empty = empty, empty_like, new_empty
    Fn._WorkspacePool.take = classmethod(take)
    try:
        yield c
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = o_empty, o_like, o_new
        Fn._WorkspacePool.take = o_take


# ---------------------------------------------------------------------------------------------- the comparison
def flatten(x, prefix="out"):
    """Every tensor inside a result (tensor, number, None, list / tuple / dict of these) as [(name, tensor)]."""
    if x is None:
        return []
    if isinstance(x, torch.Tensor):
        return [(prefix, x)]
    if isinstance(x, np.ndarray):
        return [(prefix, torch.from_numpy(np.ascontiguousarray(x)))]
    if isinstance(x, (bool, int, float, np.generic)):
        return [(prefix, torch.tensor(float(x), dtype=torch.float64))]
    if isinstance(x, dict):
        return [kv for k in x for kv in flatten(x[k], f"{prefix}.{k}")]
    if isinstance(x, (list, tuple)):
        return [kv for i, v in enumerate(x) for kv in flatten(v, f"{prefix}[{i}]")]
    raise TypeError(f"{prefix}: cannot compare a {type(x).__name__}")


_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """The logical elements of `t` as integers of the same width on the CPU: NaN equals itself, -0.0 differs from 0.0.
    (Strided views are compared over their elements only: a sliced-off pad column is not part of the result.)"""
    t = t.detach()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    t = t.contiguous().cpu()
    return t.view(_BITS[t.element_size()]) if t.numel() else t


def snapshot(result):
    return [(k, v.dtype, tuple(v.shape), bits(v).clone()) for k, v in flatten(result)]


def differences(a, b):
    """Names (with the count of differing elements) where two snapshots are not the same bits."""
    if [x[:3] for x in a] != [x[:3] for x in b]:
        return [f"layout {[x[:3] for x in a]} != {[x[:3] for x in b]}"]
    out = []
    for (k, _, _, x), (_, _, _, y) in zip(a, b):
        if not torch.equal(x, y):
            bad = (x != y)
            out.append(f"{k}: {int(bad.sum())} of {x.numel()} elements, first at flat index {int(bad.reshape(-1).nonzero()[0])}")
    return out


def fill_dependence(fn, spare_pool=(), sync=None):
    """Run fn() plain and under every fill -> (report, counters, result under 0xFF).  report: one line per (fill, tensor) whose
    bits differ from the plain run - empty when no result depends on what uninitialised memory held.  counters: fill -> Counters.
    sync: called after each run, before its result is read (torch.cuda.synchronize on the GPU)."""
    def once():
        r = fn()
        if sync is not None:
            sync()
        return r
    plain = snapshot(once())
    report, counters, last = [], {}, None
    for byte in FILLS:
        with poisoned(byte, spare_pool) as c:
            last = once()
            got = snapshot(last)
        counters[byte] = c
        report += [f"fill 0x{byte:02X}: {d}" for d in differences(plain, got)]
    return report, counters, last
