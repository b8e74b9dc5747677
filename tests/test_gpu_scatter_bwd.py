"""f2n_scatter_add_bwd (scatter.hip) against exact integer sums (tests/step_tail_cases.py): dsum holds
multiples of 2^-10 few enough per image that every f32 partial sum is exact, so the kernel's atomics
must give the int64 reference bit for bit -- at id runs that start, end and cross the 64-sample spans,
channel counts that are no power of two, ids outside [0, n_emb) and images no sample names."""
import numpy as np
import pytest
import torch

from tests import step_tail_cases as st

pytestmark = pytest.mark.gpu

CASES = [(n, C) for n in st.SCATTER_N for C in st.SCATTER_C]


def _call(capi, dev, case, n_all, C):
    ids = torch.from_numpy(case["ids"]).to(dev)
    dsum = torch.from_numpy(case["dsum"]).to(dev)
    demb = torch.full((st.SCATTER_E * C + st.GUARD,), st.SENTINEL, device=dev)   # pre-filled: overwritten
    capi.call("scatter_add_bwd", ids, dsum, demb, n_all, st.SCATTER_E, C)
    torch.cuda.synchronize()
    return demb.cpu().numpy()


@pytest.mark.parametrize("n_all,C", CASES)
def test_scatter_add_bwd_exact(capi, dev, n_all, C):
    case = st.scatter_case(n_all, C)
    got = _call(capi, dev, case, n_all, C)
    st.assert_none(st.scatter_failures(case, got), "n_all=%d C=%d" % (n_all, C))
    again = _call(capi, dev, case, n_all, C)
    assert np.array_equal(got.view(np.int32), again.view(np.int32))
    print("[step-tail] scatter_add_bwd n_all=%d C=%d: %d of %d elements non-zero, all exact" % (
        n_all, C, int((got[:st.SCATTER_E * C] != 0).sum()), st.SCATTER_E * C))


def test_scatter_add_bwd_no_samples_zeroes_demb(capi, dev):
    """n_all == 0: the rows are still overwritten with +0, nothing past them is touched"""
    C = 3
    demb = torch.full((st.SCATTER_E * C + st.GUARD,), st.SENTINEL, device=dev)
    ids = torch.zeros(1, dtype=torch.int32, device=dev)
    capi.call("scatter_add_bwd", ids, torch.zeros(1, C, device=dev), demb, 0, st.SCATTER_E, C)
    got = demb.cpu().numpy()
    assert (got[:st.SCATTER_E * C].view(np.int32) == 0).all()
    assert (got[st.SCATTER_E * C:] == np.float32(st.SENTINEL)).all()
