#!/usr/bin/env python3
"""
G14: the reference's own recon/regularized.py::RegularizedRecon run on G5's sinogram (32^3, 16 angles; read from g5_sirt.npz, not
duplicated) -- two cases per method.  Imports make_golden for its shims (numpy index_tricks, scipy.optimize.linesearch) and helpers.

The reference class does not run as written; adapted from OUTSIDE, without editing it:
  * obj.my_rank = 0 (the serial class reads it in its stop rule, :117, :211, :387);
  * run_lasso_ista calls plt.figure() unconditionally (:312-314), and plt is a local imported under make_plot: it runs with
    make_plot=True against a no-op matplotlib.pyplot placed in sys.modules;
  * my_tikh_f is replaced by a wrapper that counts its calls and ravels b (A x - b with the 2-D sinogram does not broadcast, :418);
    the per-iteration counts come from a pass-through around line_search_armijo (its f_count);
  * run_lasso_ista's step_size is a local: the no-op plt.plot records it (:313).
Written: g14_regularized_solvers.npz with, per case, rec (float32), rms, k, the parameters, ISTA's step_size and the Tikhonov line
search's evaluation counts.  Run in the authoring container:  oracle/build_ref.sh && python tests/golden/make_golden_g14.py
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shims + reference on sys.path)
import numpy as np  # noqa: E402
from recon import regularized  # noqa: E402
from utilities import generate_phantom  # noqa: E402

# (tag, method, kwargs, ground truth?, warm start?)
CASES = [
    ("fista_a", "run_fista", dict(niter=12, hyper=2.e3, beta_tv=0.5, niter_tv=20), False, False),
    ("fista_b", "run_fista", dict(niter=30, hyper=1.e3, beta_tv=20.0, niter_tv=10), True, False),
    ("tikh_a", "run_tikhonov_gd", dict(niter=8, reg_param=1.0, positivity=True), False, False),
    ("tikh_b", "run_tikhonov_gd", dict(niter=30, reg_param=300.0, positivity=True), True, True),
    ("ista_a", "run_lasso_ista", dict(niter=8, reg_param=0.5, alpha0=1.0, beta=0.5), False, False),
    ("ista_b", "run_lasso_ista", dict(niter=30, reg_param=20.0, alpha0=0.05, beta=0.5), True, True),
    ("acc_a", "run_lasso_accelerated", dict(niter=8, reg_param=0.5, alpha0=1.0, beta=0.5), False, False),
    ("acc_b", "run_lasso_accelerated", dict(niter=30, reg_param=20.0, alpha0=0.01, beta=0.8), True, True),
]


def warm_start(N):
    return (0.5 * generate_phantom.shepp3d(N)).astype(np.float32).ravel()


def main():
    g5 = np.load(os.path.join(HERE, "g5_sirt.npz"))
    N, n_proj = 32, 16
    geo = mg.geom(n_proj, N)
    angles = np.array([g5["phi"], g5["alpha"], g5["beta"]]).T
    x = generate_phantom.shepp3d(N).astype(np.float32)
    plotted = []          # run_lasso_ista's local step_size reaches the outside only through its closing plt.plot(step_size) (:313)

    class _Nop(object):
        def __getattr__(self, name):
            return lambda *a, **k: _Nop()

        def __iter__(self):
            return iter([_Nop() for _ in range(3)])

    fake = types.ModuleType("matplotlib.pyplot")
    fake.__getattr__ = lambda name: (lambda *a, **k: _Nop())
    fake.subplots = lambda *a, **k: (_Nop(), _Nop())
    fake.plot = lambda a, *r, **k: plotted.append(np.array(a))
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = fake
    sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, fake
    orig_f, orig_ls = regularized.my_tikh_f, regularized.line_search_armijo
    n_f, per_iter = [0], []

    def counting_f(xx, A, b, lam):
        n_f[0] += 1
        return orig_f(xx, A, np.ravel(b), lam)

    def ls(*a, **kw):
        out = orig_ls(*a, **kw)
        per_iter.append(out[1])
        return out

    regularized.my_tikh_f, regularized.line_search_armijo = counting_f, ls
    out = {}
    try:
        for tag, meth, kw, with_gt, warm in CASES:
            opts = {}
            if with_gt:
                opts["ground_truth"] = x.ravel().copy()
            if warm:
                opts["rec"] = warm_start(N)
            obj = regularized.RegularizedRecon(geo, g5["b"].copy(), angles, g5["xyz"], options=opts)
            obj.my_rank = 0
            n_f[0], per_iter[:] = 0, []
            # plt is a LOCAL of run_lasso_ista (imported under make_plot): its closing plt.figure() runs only with make_plot set
            rec, rms = getattr(obj, meth)(make_plot=(meth == "run_lasso_ista"), **kw)
            out[tag + "_rec"] = np.asarray(rec, np.float32)
            out[tag + "_rms"] = np.asarray(rms, np.float64)
            out[tag + "_k"] = np.array(len(rms))
            if meth == "run_lasso_ista":
                out[tag + "_step_size"] = np.asarray(plotted.pop(), np.float64)
            if meth == "run_tikhonov_gd":
                out[tag + "_n_feval"] = np.array(per_iter, np.int64)
                out[tag + "_n_feval_total"] = np.array(n_f[0])
            print("   g14 %-8s k %2d of %2d  rms %s  %s" % (tag, len(rms), kw["niter"], np.array2string(np.asarray(rms), precision=5, max_line_width=200),
                                                       ("fevals %s" % per_iter) if per_iter else ""))
    finally:
        regularized.my_tikh_f, regularized.line_search_armijo = orig_f, orig_ls
    mg.save("g14_regularized_solvers", **out)


if __name__ == "__main__":
    main()
