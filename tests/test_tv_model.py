"""tests/tv_model.py against the oracle and the reference's own outputs (golden G9), and the conditions on its case table that keep
the GPU tests of the TV proximal step (tests/test_gpu_tv_prox.py) from hiding a failure: the stop of every case with eps > 0 is
decided by a margin far above what float32 does to a gap, and the cases marked exact never project (so their iteration is adds and
products only and float32 results are comparable bit for bit)."""
import numpy as np
import pytest

import tv_model as tm
from conftest import golden, rel_max

G9_CASES = {"a": dict(weight=0.2, niter=20, eps=0.0, check_gap_frequency=3), "b": dict(weight=0.05, niter=200, eps=1.e-3, check_gap_frequency=3),
            "c": dict(weight=0.5, niter=1, eps=0.0, check_gap_frequency=1), "d": dict(weight=0.5, niter=0, eps=1.e-5, check_gap_frequency=3)}
G9_ITERS = {"a": 20, "b": 6, "c": 1, "d": 0}


@pytest.mark.parametrize("case", tm.CASES, ids=tm.CASE_IDS)
def test_float64_model_is_the_oracle(case):
    from oracle import oracle as orc
    new, iters, gap = tm.case_model(case, np.float64)[:3]
    want, want_iters, want_gap = orc.tv_denoise_fista(tm.case_input(case).astype(np.float64), return_info=True, **tm.params(case))
    assert iters == want_iters
    assert new.dtype == np.float64 and np.max(np.abs(new - want)) <= 1e-12
    assert abs(gap - want_gap) <= 1e-12


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_reproduces_g9(dtype):
    g = golden("g9_regularized")
    for tag, kw in G9_CASES.items():
        new, iters = tm.denoise_fista(g["tv_im"], dtype=dtype, **kw)[:2]
        assert iters == G9_ITERS[tag], (tag, iters)
        assert new.dtype == dtype and rel_max(new, g["tv_" + tag]) < 1e-5, tag
        if tag == "d":
            assert np.array_equal(new, g["tv_im"].astype(dtype))


@pytest.mark.parametrize("case", tm.CASES, ids=tm.CASE_IDS)
def test_stop_margin(case):
    """Every checked gap of the float64 model is at least 1e-2 eps away from eps, and float32 moves a gap by far less: the number of
    iterations is decided, so the GPU tests demand it exactly."""
    eps = tm.params(case)["eps"]
    m64, m32 = tm.case_model(case, np.float64), tm.case_model(case, np.float32)
    assert m32[1] == m64[1] and len(m32[3]) == len(m64[3])
    if eps > 0:
        margin = min(abs(g - eps) for g in m64[3]) / eps
        moved = max(abs(a - b) for a, b in zip(m32[3], m64[3])) / eps
        print("%s: %d iterations, smallest |gap - eps| / eps %.2e, largest float32 effect on a gap %.2e eps" % (tm.case_id(case), m64[1], margin, moved))
        assert margin >= 1e-2
        assert moved < 1e-1 * margin
        assert 0 < m64[1] < tm.params(case)["niter"]          # the stop rule, not niter, ended it


@pytest.mark.parametrize("case", tm.EXACT, ids=[tm.case_id(c) for c in tm.EXACT])
def test_exact_regime(case):
    """No dual vector comes near the unit ball: max(sqrt(q), 1) is 1, the division is by 1."""
    for dtype in (np.float32, np.float64):
        worst = tm.case_model(case, dtype)[4]
        assert 0.0 < worst < 0.5, (dtype, worst)


def test_case_table():
    assert len(tm.CASES) == 26 and len(set(tm.CASE_IDS)) == 26
    assert [s for t, s in tm.CASES if s == tm.BIG and t in "AC"] == []
    assert np.prod(tm.BIG) == 2048 * 256 + 32
    x = tm.block((16, 12, 20))
    assert x.dtype == np.float32 and abs(float(x[4:12, :, 4:16].mean()) - 1.0) < 0.05 and abs(float(x[:4].mean())) < 0.05
    f = tm.flat((5, 4, 255))
    assert f.dtype == np.float32 and 0.0 <= f.min() and f.max() < 1.0
