"""Every output of the embedding ops (neighbors, clusters, latent_gaussian) as one .npz - to be run with two builds of the library
(RR_LIB_PATH) on one MI355X and compared byte for byte:
    python tools/embedding_bits.py --out A.npz
    python tools/embedding_bits.py --compare A.npz B.npz    (prints the array count and the names that differ; status 1 on any)
Per seed, a pool of 3000 rows with every row twice (ties in every distance, score and key) at widths 37, 300 and 1100 (1000 for
the moments, which stop at 1024), each as a 16-byte aligned view of a padded buffer and as a view one float further (4-byte
loads): row_sqnorm; knn (k = 16) and radius_count (with and without groups) with the splits pinned to 0, 1 and 7;
kcenter_greedy plain and weighted and sphere_exclusion in both orders, to the end (batched continuation) and with
max_clusters = 70, with the blocks pinned to 0 and 3; latent_gaussian.scatter and center_project (y and sq) likewise.  Every
knob is reset afterwards.
    python tools/embedding_bits.py --host --out A.npz       needs no GPU: every rr_*_workspace_bytes of these ops,
rr_moments_chunks and rr_knn_geometry over a grid of shapes (0, 1, tile edges, 10^6, 2^31 - 1 and 2^31), at every pin."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from reactranker_amd import clusters as CL  # noqa: E402
from reactranker_amd import latent_gaussian as LG  # noqa: E402
from reactranker_amd import neighbors as NB  # noqa: E402
from reactranker_amd._lib import lib  # noqa: E402
from tools.window_loss_bits import compare  # noqa: E402

SEEDS = (0, 1)
WIDTHS = (37, 300, 1100)
ROWS, QUERIES = 3000, 257
SPLITS, BLOCKS = (0, 1, 7), (0, 3)
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 10 ** 6, 2 ** 31 - 1, 2 ** 31)
OUT = {}


def put(name, x):
    assert name not in OUT, name
    OUT[name] = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def put_all(name, d):
    for k, v in (d.items() if isinstance(d, dict) else enumerate(d)):
        if v is not None:
            put(f"{name}/{k}", v)


def knobs(splits=0, blocks=0):
    l = lib()
    assert l.rr_knn_set_splits(splits) == 0
    for setter in (l.rr_kcenter_set_blocks, l.rr_sphere_exclusion_set_blocks, l.rr_moments_set_blocks, l.rr_resample_set_blocks):
        assert setter(blocks) == 0


def view(host, offset):
    """the [rows, H] matrix as a view of a buffer with a pitch % 4 == 0, its first element `offset` floats past a 16-byte boundary"""
    n, H = host.shape
    W = (H + 3) // 4 * 4 + 4
    flat = torch.zeros(n * W + 4, dtype=torch.float32, device="cuda")
    x = flat[offset:offset + n * W].view(n, W)[:, :H]
    x.copy_(torch.from_numpy(host))
    assert x.data_ptr() % 16 == 4 * offset
    return x


def pool_of(seed, H):
    rng = np.random.default_rng(100 * seed + H)
    x = np.round(rng.standard_normal((ROWS, H)) * 2).astype(np.float32) / 2
    x[ROWS // 2:] = x[:ROWS // 2]                                    # every row twice
    return rng, x


def search_outputs(seed, H, offset):
    rng, host = pool_of(seed, H)
    x = view(host, offset)
    tag = f"s{seed}/h{H}/o{offset}"
    radius = float(np.sqrt(1.9 * H))                                 # about the typical distance of two rows: both sides of r2 occur
    g = torch.arange(ROWS, dtype=torch.int32) % 50
    w = torch.tensor((1 + rng.integers(0, 3, ROWS)).astype(np.float32)).cuda()
    put(tag + "/row_sqnorm", NB.row_sqnorm(x))
    for s in SPLITS:
        knobs(splits=s)
        put_all(f"{tag}/knn/s{s}", NB.knn(x[:QUERIES], x, 16))
        put(f"{tag}/radius_count/s{s}", CL.radius_count(x[:QUERIES], x, radius))
        put(f"{tag}/radius_count_groups/s{s}", CL.radius_count(x[:QUERIES], x, radius, q_group=g[:QUERIES], b_group=g))
    for b in BLOCKS:
        knobs(blocks=b)
        put_all(f"{tag}/kcenter/b{b}", NB.kcenter_greedy(x, 65))
        put_all(f"{tag}/kcenter_weighted/b{b}", NB.kcenter_greedy(x, 65, weight=w))
        for order in CL.ORDERS:
            put_all(f"{tag}/sphere_exclusion/{order}/b{b}", CL.sphere_exclusion(x, radius, order=order))
            put_all(f"{tag}/sphere_exclusion/{order}/b{b}/n70", CL.sphere_exclusion(x, radius, order=order, max_clusters=70))


def gaussian_outputs(seed, H, offset):
    rng, host = pool_of(seed, H)
    host[5, 0], host[77, H - 1] = np.nan, np.inf                     # two rows the moments leave out
    x = view(host, offset)
    tag = f"s{seed}/h{H}/o{offset}"
    center = torch.tensor(rng.standard_normal(H).astype(np.float32)).cuda()
    W = torch.tensor(rng.standard_normal((H, min(H, 40))).astype(np.float32)).cuda()
    for b in BLOCKS:
        knobs(blocks=b)
        put_all(f"{tag}/scatter/b{b}", LG.scatter(x))
        put_all(f"{tag}/center_project/b{b}", LG.center_project(x, center, W, want_y=True, want_sq=True))
        put(f"{tag}/center_project_sq_only/b{b}", LG.center_project(x, None, W, want_y=False, want_sq=True)[1])


def host_outputs():
    l = lib()
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    l.rr_knn_geometry(C.byref(a), C.byref(b), C.byref(c))
    put("knn_geometry", [a.value, b.value, c.value])

    def sized(fn, *shape):                                           # (status, bytes; bytes -1 where the entry refuses)
        n = C.c_size_t(0)
        st = fn(*shape, C.byref(n))
        return [st, n.value if st == 0 else -1]
    for s in SPLITS:
        knobs(splits=s)
        put(f"knn_workspace_bytes/s{s}", np.array([[[sized(l.rr_knn_workspace_bytes, M, N, k) for k in (1, 16, 64, 65)]
                                                      for N in SIZES] for M in SIZES], np.int64))
        put(f"radius_count_workspace_bytes/s{s}", np.array([[sized(l.rr_radius_count_workspace_bytes, M, N) for N in SIZES]
                                                             for M in SIZES], np.int64))
    for blocks in BLOCKS:
        knobs(blocks=blocks)
        put(f"kcenter_workspace_bytes/b{blocks}", np.array([[sized(l.rr_kcenter_workspace_bytes, P, n) for n in (0, 1, 65536, 65537)]
                                                            for P in SIZES], np.int64))
        put(f"sphere_exclusion_workspace_bytes/b{blocks}", np.array([sized(l.rr_sphere_exclusion_workspace_bytes, P) for P in SIZES],
                                                                     np.int64))
        widths = (1, 63, 64, 65, 300, 1000, 1023, 1024, 1025)
        put(f"moments_workspace_bytes/b{blocks}", np.array([[sized(l.rr_moments_workspace_bytes, N, H) for H in widths]
                                                            for N in SIZES], np.int64))
        put(f"moments_chunks/b{blocks}", np.array([[l.rr_moments_chunks(N, H) for H in widths] for N in SIZES], np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, metavar="NPZ", default=None)
    ap.add_argument("--host", action="store_true", help="the host-side sizing functions only (no GPU)")
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if not args.out:
        ap.error("--out FILE is required unless --compare is given")
    try:
        if args.host:
            host_outputs()
        else:
            for seed in SEEDS:
                for H in WIDTHS:
                    for offset in (0, 1):
                        search_outputs(seed, H, offset)
                        gaussian_outputs(seed, min(H, 1000), offset)
    finally:
        knobs()
    np.savez(args.out, **OUT)
    print(f"{len(OUT)} arrays -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
