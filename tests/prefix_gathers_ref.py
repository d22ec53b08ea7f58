"""numpy restatement of the two shared-prefix gathers of csrc/gather.hip, COMPOSED from the restatements of the launches they
replace (tests/gather_ref.py, imported as is):

  gather2_sum_dropmask = gather_sum into the intermediate, its row 0 replaced by the sum of the partial rows, then
                         gather_sum_dropmask over the intermediate
  gather_sum_dropsrc   = gather_dropout into the copies, then gather_sum over the copies

TEST INFRASTRUCTURE: nothing here is on the product path."""
import numpy as np

from tests import gather_ref as R

F32 = np.float32


def gather2_sum_dropmask(src, in_idx, y, scale, out_idx, H, p, seed, row0=None):
    """row0: what the padding-row reduction stored in intermediate row 0 ([H] floats; the tree sum is not restated here -
    the GPU tests take it from rr_gather_sum_padrow_f32, the CPU test from a single partial row)."""
    mid = R.gather_sum(src, in_idx, H)
    if row0 is not None:
        mid[0, :] = np.asarray(row0, F32)[:H]
    return R.gather_sum_dropmask(mid, y, scale, out_idx, H, p, seed)


def gather_sum_dropsrc(y, copies, idx, H, p, seed):
    return R.gather_sum(R.gather_dropout(y, copies, H, p, seed), idx, H)
