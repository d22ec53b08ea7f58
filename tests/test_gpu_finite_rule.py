"""The finite rule of the embedding ops (csrc/row_chain.h: rr_finite over the H columns of a row, read by rr_load4) gives one
answer through the three ops that share it - kcenter_greedy (min_dist NaN), sphere_exclusion (label -2) and the moments (rows
left out) - at every width class of the kernels, with 16-byte and with 4-byte loads, and whatever the pitch padding holds."""
import numpy as np
import pytest
import torch

from reactranker_amd import clusters as K
from reactranker_amd import latent_gaussian as G
from reactranker_amd import neighbors as N
from reactranker_amd._lib import lib

pytestmark = pytest.mark.gpu

P = 9                                                      # with one workgroup of four waves: three grid passes
NAN, INF = float("nan"), float("inf")
# (row, column: 0 = the first, -1 = the last of the H, value); rows 0, 4 and 8 are clean
BAD = ((1, 0, NAN), (2, -1, INF), (3, 0, -INF), (5, -1, NAN), (6, 0, INF), (7, -1, -INF))
PADDED_ROW = 4                                             # clean, but NaN in the pitch padding just past column H - 1


def _pool(H, offset):
    """(x: the [P, H] view of a wider buffer whose first element lies `offset` floats past a 16-byte boundary, good [P] bool)"""
    W = (H + 1 + 3) // 4 * 4                               # pitch % 4 == 0 and at least one padding column
    rng = np.random.default_rng(1000 * H + offset)
    host = rng.standard_normal((P, W)).astype(np.float32)
    for r, c, v in BAD:
        host[r, c if c == 0 else H - 1] = v
    host[PADDED_ROW, H:] = NAN
    flat = torch.zeros(P * W + 4, dtype=torch.float32, device="cuda")
    flat[offset:offset + P * W] = torch.from_numpy(host.reshape(-1)).cuda()
    x = flat[offset:offset + P * W].view(P, W)[:, :H]
    assert x.data_ptr() % 16 == 4 * offset and x.stride(0) == W
    return x, np.isfinite(host[:, :H]).all(axis=1)


@pytest.mark.parametrize("offset", (0, 1), ids=("aligned", "offset1"))
@pytest.mark.parametrize("H", (1, 5, 260, 1024, 1028))     # NG = 1, 1, 2, 4 and the loop for wider rows (kcenter, cluster only)
def test_one_finite_rule_through_kcenter_clusters_and_moments(H, offset):
    x, good = _pool(H, offset)
    assert good.tolist() == [r in (0, PADDED_ROW, 8) for r in range(P)]
    l = lib()
    try:
        assert l.rr_kcenter_set_blocks(1) == 0 and l.rr_sphere_exclusion_set_blocks(1) == 0
        min_dist = N.kcenter_greedy(x, 0)["min_dist"].cpu().numpy()
        labels = K.sphere_exclusion(x, 1.0, order="index", max_clusters=0)["labels"].cpu().numpy()
    finally:
        assert l.rr_kcenter_set_blocks(0) == 0 and l.rr_sphere_exclusion_set_blocks(0) == 0
    print(f"H {H} offset {offset}: min_dist {min_dist.tolist()} labels {labels.tolist()}")
    assert (np.isnan(min_dist) == ~good).all() and (min_dist[good] == INF).all()
    assert (labels == np.where(good, -1, -2)).all()
    if H <= G.MAX_H:
        n_used = int(G.scatter(x)[2])
        print(f"  n_used {n_used}")
        assert n_used == int(good.sum())
