"""The rows of tests/build_cases.py that a small shape reaches, through the real entry points.

Two fp32 tables of 3 and 5000 rows, dim 16, uniform indices; per row of build_cases.GPU_CASES one call of its entry
point (dlrm_indexer_build -- pooled as B x 4 where N divides --, dlrm_indexer_build_split, dlrm_indexer_prepare,
dlrm_step_fwd, dlrm_step_bwd_prepare), then:
  - the return code and the dlrm_indexer_state bits the row's plan implies (BUILT, SPLIT where the build is split,
    PREPARED from the two sites that prepare, no SINGLES bit);
  - helpers._assert_segments on both tables: exact;
  - the once-hit flags: an update of all-zero tables with this build (DLRM_UPDATE_PREBUILT), a gradient of ones and
    lr = 1 must leave row r at minus its np.unique count, all 16 columns -- exact in fp32; a split build lists no
    once-hit row, so a count of one is right only if its position was flagged, and a flag on a repeated row's
    position would step that row twice.
Nothing here has a tolerance.  The 2^20 + 1 rows are taken too: dlrm_indexer_build's sorted unsplit kernel (the
parent's library passes the row in 0.6 s) and dlrm_indexer_build_split's refusal, DLRM_E_UNSUPPORTED with the
indexer untouched.

tools/launch_trace.py runs the same rows for a kernel trace; profiles/build_plan/forms_parent_lib.txt is this
module's run against the parent's library.
"""
import numpy as np
import pytest
import torch

import build_cases
from helpers import _assert_segments

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", build_cases.GPU_CASES)
def test_form_through_entry_point(pkg, gpu, name):
    case = build_cases.BY_NAME[name]
    lib = pkg._lib
    form, _kind, _vshift, split, _has_map, _err, _side, want_rc = case.expected
    rc, ix, idx, p, ts = build_cases.drive(pkg, gpu, case)
    print(f"{name}: rc {rc} state {ix.state():#x}")
    assert rc == want_rc
    if form == "none":  # refused: nothing launched, the (fresh) indexer holds no build
        assert rc == lib.E_UNSUPPORTED and ix.state() == 0
        ts.ctx.check_bounds()
        return
    prepared = case.site in ("prepare", "in_apply") and form == "wave"
    assert ix.state() == lib.IX_BUILT | (lib.IX_SPLIT if split else 0) | (lib.IX_PREPARED if prepared else 0)
    ts.ctx.check_bounds()
    _assert_segments(ix, idx, case.N)
    if not split:  # (the sorted unsplit kernel lists every row: no flags)
        return
    # the once-hit flags, through the update that reads them
    for t in ts:
        t.data.zero_()
    B = case.N // case.L
    hp = pkg.HotPath(ts, B, case.L, lr=1.0, index_base=0)
    hp.indexer = ix
    hp.dt.fill_(1.0)
    hp.sgd_update(p, True)
    torch.cuda.synchronize()
    ts.ctx.check_bounds()
    for t, n in enumerate(build_cases.GPU_ROWS):
        want = -np.bincount(idx[t], minlength=n).astype(np.float32)
        got = ts[t].data.cpu().numpy()
        assert np.array_equal(got, np.repeat(want[:, None], build_cases.GPU_DIM, axis=1)), (name, t)
        assert (want == -1).any() or n < 10  # (the large table has once-hit rows: the flags were exercised)
