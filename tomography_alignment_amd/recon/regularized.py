"""
The reference's recon/regularized.py: the class RegularizedRecon (TV-FISTA, Tikhonov gradient descent with an Armijo line search,
LASSO by ISTA with backtracking and its accelerated form; :13-413), the module-level cost / gradient of the Tikhonov problem
my_tikh_f / my_tikh_fp (:416-431) and soft_thresholding (:433-440), with the reference's signatures.

RegularizedRecon runs device-resident: the iterate, the gradient, the trial points of the line searches and the TV proximal step live
in HBM; per iteration only scalars cross PCIe (one accumulator fetch per reduction point; csrc/tomo_reg.hip's fused passes produce
them), and run_* downloads the reconstruction once at the end.  `self.d_rec` holds it on the device.

Decisions on the reference's defects (it does not run as written):
  * scipy.optimize.linesearch.line_search_armijo (:8) no longer exists: scipy's scalar_search_armijo is restated below
    (c1 = 1e-4, alpha0 = 1, amin = 0; quadratic, then cubic interpolation; None when it fails) and driven on device trial points;
  * the serial class reads self.my_rank (:117, :211, :387), which only the MPI class defines: here it behaves as rank 0 -- it prints
    and stops;
  * run_lasso_ista calls plt.figure() unconditionally (:312-314): there is no plotting; make_plot is accepted and ignored with a
    message, on every method;
  * `voxel_mask` is stored but never given to the projector (:36, :54): ignored here too (recon/sirt.py's SIRT, unlike this class,
    passes it on);
  * my_tikh_f subtracts the 2-D sinogram from the flat A x (:418), which does not broadcast: my_tikh_f / my_tikh_fp below ravel b,
    as recon/sirt.py's my_f does.
`precision` is accepted and recorded; the device computes in float32 (as SIRT and CGLS here do).

Angle-sharded twin: recon/regularized_mpi.py (the hooks _my_rows / _local_geometry / _allreduce_vol / _scalars / _is_root).
"""
import numpy as np

try:
    from .. import _lib
    from ..utilities import projection_operators
    from ..utilities import tv_denoise as _tv
except ImportError:      # imported as top-level `recon`
    import _lib
    from utilities import projection_operators
    from utilities import tv_denoise as _tv

_NO_PLOT = 'make_plot is not supported on the device-resident solver; ignoring'


def scalar_search_armijo(phi, phi0, derphi0, c1=1e-4, alpha0=1, amin=0):
    """scipy.optimize's Armijo backtracking (Wright & Nocedal, Numerical Optimization, 1999, pp. 56-57), restated: alpha0 first, then
    the minimiser of a quadratic interpolant, then cubic interpolation until phi(alpha) <= phi0 + c1 alpha derphi0.
    -> (alpha, phi(alpha)), or (None, last phi) when alpha drops to amin.  The returned alpha is always the last one evaluated."""
    phi_a0 = phi(alpha0)
    if phi_a0 <= phi0 + c1 * alpha0 * derphi0:
        return alpha0, phi_a0
    alpha1 = -(derphi0) * alpha0 ** 2 / 2.0 / (phi_a0 - phi0 - derphi0 * alpha0)
    phi_a1 = phi(alpha1)
    if phi_a1 <= phi0 + c1 * alpha1 * derphi0:
        return alpha1, phi_a1
    while alpha1 > amin:
        factor = alpha0 ** 2 * alpha1 ** 2 * (alpha1 - alpha0)
        a = alpha0 ** 2 * (phi_a1 - phi0 - derphi0 * alpha1) - alpha1 ** 2 * (phi_a0 - phi0 - derphi0 * alpha0)
        a = a / factor
        b = -alpha0 ** 3 * (phi_a1 - phi0 - derphi0 * alpha1) + alpha1 ** 3 * (phi_a0 - phi0 - derphi0 * alpha0)
        b = b / factor
        alpha2 = (-b + np.sqrt(abs(b ** 2 - 3 * a * derphi0))) / (3.0 * a)
        phi_a2 = phi(alpha2)
        if phi_a2 <= phi0 + c1 * alpha2 * derphi0:
            return alpha2, phi_a2
        if (alpha1 - alpha2) > alpha1 / 2.0 or (1 - alpha2 / alpha1) < 0.96:
            alpha2 = alpha1 / 2.0
        alpha0 = alpha1
        alpha1 = alpha2
        phi_a0 = phi_a1
        phi_a1 = phi_a2
    return None, phi_a1


class RegularizedRecon(object):
    """Iterative reconstruction with a TV (run_fista), Tikhonov (run_tikhonov_gd) or L1 (run_lasso_ista, run_lasso_accelerated)
    penalty -- recon/regularized.py:13-413.  Options: ground_truth, precision (recorded; the device computes in float32), rec (warm
    start: numpy or DeviceArray), voxel_mask (ignored, as the reference does) and _backend (test seam; None -> HipBackend)."""

    # accumulator slots: sums over this rank's sinogram rows first (summed over the ranks), then whole-volume sums (identical on every rank);
    # _JUNK takes the sum of a pass whose scalar nobody reads
    _JUNK = 15

    def __init__(self, geometry, projections, angles, xyz_shifts, options={}):
        self.geometry = geometry
        self.projections = projections
        self.angles = angles
        self.xyz_shifts = xyz_shifts
        self.n_proj = angles.shape[0]
        self.ground_truth = options['ground_truth'] if 'ground_truth' in options else None
        self.precision = options['precision'] if 'precision' in options else np.float32
        self.rec = options['rec'] if 'rec' in options else None
        self.voxel_mask = options['voxel_mask'] if 'voxel_mask' in options else None      # stored, never used (regularized.py:36,54)
        self._backend = options.get('_backend')
        self.f_proj_obj = None
        self.proj_mat = None
        self.rms_error = None
        self.step_size = None
        self.n_feval = None
        self._initialize()

    # ---- hooks the sharded subclass overrides
    def _my_rows(self):
        return np.arange(self.n_proj)

    def _local_geometry(self, rows):
        return self.geometry

    def _allreduce_vol(self, buf):
        return buf

    def _is_root(self):
        return True

    def _scalars(self, n_row, n_vol):
        """Slots [0, n_row) summed over the ranks, then [n_row, n_row + n_vol) as this rank has them: one host synchronisation here."""
        v = self.be.acc_fetch(0, n_row + n_vol)
        return [float(x) for x in v]

    # ---- set-up
    def _initialize(self):
        rows = self._rows = self._my_rows()
        if self.f_proj_obj is None:
            self.f_proj_obj = projection_operators.ProjectionMatrix(self._local_geometry(rows), precision=self.precision, backend=self._backend)
            self.proj_mat = self.f_proj_obj.projection_matrix(phi=self.angles[rows, 0], alpha=self.angles[rows, 1], beta=self.angles[rows, 2],
                                                              xyz_shift=self.xyz_shifts[rows])
        be = self.be = self.f_proj_obj.backend
        self.n_vox, n_rows = be.n_vox, int(np.size(rows)) * be.n_det
        self.vox_shape = tuple(int(v) for v in self.geometry.vox_shape)
        if self.rec is None:
            self.d_rec = be.zeros(self.n_vox)
        else:
            self.d_rec = be.empty(self.n_vox)
            if be.is_buffer(self.rec):
                be.copy(self.d_rec, self.rec)
            else:
                self.d_rec.upload(np.asarray(self.rec, np.float32).ravel())
        if be.is_buffer(self.projections):              # already in HBM: this rank's rows
            self.d_b = self.projections
        else:
            self.d_b = be.upload(np.asarray(self.projections, np.float32).reshape(self.n_proj, -1)[rows])
        self.d_ax = be.empty(n_rows)
        self.d_res = be.empty(n_rows)
        self.d_bp = be.empty(self.n_vox)
        self.d_tmp = be.empty(self.n_vox)               # trial points / the TV prox output / x_0 of the accelerated method
        self.d_tmp2 = None                               # allocated by the methods that need a third volume
        self.d_gt = None
        if self.ground_truth is not None:
            self.d_gt = self.ground_truth if be.is_buffer(self.ground_truth) else be.upload(np.asarray(self.ground_truth, np.float32).ravel())
        self.norm_factor = self._norm_factor()

    def _norm_factor(self):
        """||gt|| or ||b|| (all rows) -- regularized.py:38-43."""
        be = self.be
        if self.ground_truth is not None and not be.is_buffer(self.ground_truth):
            return float(np.linalg.norm(np.asarray(self.ground_truth, np.float64)))
        if self.ground_truth is None and not be.is_buffer(self.projections):
            return float(np.linalg.norm(np.asarray(self.projections, np.float64)))
        be.acc_zero(0, 2)
        if self.ground_truth is not None:                # device gt: deterministic ||gt - 0||^2, the same on every rank
            be.fill(self.d_tmp, 0.0)
            be.clamp_err(self.d_tmp, False, self.d_gt, slot=1)
            return float(np.sqrt(self._scalars(0, 2)[1]))
        be.fill(self.d_ax, 0.0)
        be.residual_acc(None, self.d_b, self.d_ax, slot=0)
        return float(np.sqrt(self._scalars(1, 0)[0]))

    def _vol2(self):
        if self.d_tmp2 is None:
            self.d_tmp2 = self.be.empty(self.n_vox)
        return self.d_tmp2

    def _residual_and_backprojection(self, negate):
        """d_res = +-(A rec - b) with ||res||^2 into slot 0; d_bp = A^T d_res summed over the ranks (the one volume all-reduce)."""
        be = self.be
        self.proj_mat.apply(self.d_rec, self.d_ax)
        be.residual_acc(self.d_res, self.d_ax, self.d_b, negate=negate, slot=0)
        self.proj_mat.T.apply(self.d_res, self.d_bp)
        self._allreduce_vol(self.d_bp)

    def _semi_converged(self, k, rms_error, after):
        if k > after and rms_error[k] > rms_error[k - 1]:
            if self._is_root():
                print('semi-convergence criterion reached: stopping at k %3d with RMSE = %4.5f' % (k, rms_error[k]))
            return True
        return False

    def _finish(self, rms_error, k):
        self.rms_error = rms_error
        self.rec = self.be.download(self.d_rec)
        return self.rec, rms_error[:k]

    # ---- TV-FISTA                                                                                  regularized.py:57-154
    def run_fista(self, niter=100, make_plot=False, hyper=1.e4, beta_tv=1.0, niter_tv=20):
        if make_plot:
            print(_NO_PLOT)
        be = self.be
        gamma = 1. / hyper
        t = 1.0
        rms_error = np.zeros(niter, )
        u, u_old = self.d_tmp, self._vol2()
        be.copy(u_old, self.d_rec)                                                  # :80
        self.tv_iters = []
        k, stop = 0, 0
        while k < niter and not stop:
            be.acc_zero(0, 2)
            self._residual_and_backprojection(negate=True)                          # :85-88  res = b - A rec ; A^T res
            be.trial(self.d_bp, self.d_rec, self.d_bp, gamma, slot=self._JUNK)      # :90  x_tmp = rec + gamma A^T res
            it, _ = be.tv_prox_det(self.d_bp, u, self.vox_shape, weight=gamma * beta_tv, niter=niter_tv)      # :93-94
            self.tv_iters.append(it)
            t_old = t
            t = 0.5 * (1.0 + np.sqrt(1 + 4 * t_old ** 2))                          # :97-98
            be.fista_momentum(self.d_rec, u, u_old, (t_old - 1) / t, self.d_gt, slot=1)      # :101-102
            u, u_old = u_old, u                                                     # :103
            res2, err2 = self._scalars(1, 1)
            data_fidelity = 0.5 * res2                                              # :106
            rms_error[k] = np.sqrt(2 * data_fidelity) / self.norm_factor if self.d_gt is None else np.sqrt(err2) / self.norm_factor
            stop = self._semi_converged(k, rms_error, 0)                           # :115-119
            k += 1
        return self._finish(rms_error, k)

    # ---- Tikhonov gradient descent with an Armijo line search                                       regularized.py:156-237
    def run_tikhonov_gd(self, niter=100, reg_param=1.0, positivity=False, make_plot=False):
        if make_plot:
            print(_NO_PLOT)
        be = self.be
        rms_error = np.zeros(niter, )
        self.n_feval = []
        trial = self._vol2()
        k, stop = 0, 0
        while k < niter and not stop:
            be.acc_zero(0, 3)
            self._residual_and_backprojection(negate=True)                          # :177-178
            be.tikh_grad(self.d_bp, self.d_rec, reg_param, slot=1)                  # :180  grad = -A^T res + lambda rec
            res2, g2, r2 = self._scalars(1, 2)
            cost = 0.5 * (res2 + reg_param * r2)                                    # :188
            last = [None, 0]

            def phi(alpha):                                                         # my_tikh_f(rec - alpha grad)   :416-422
                be.acc_zero(0, 2)
                be.trial(trial, self.d_rec, self.d_bp, -alpha, slot=1)
                self.proj_mat.apply(trial, self.d_ax)
                be.residual_acc(None, self.d_ax, self.d_b, slot=0)
                last[0], last[1] = alpha, last[1] + 1
                s_res, s_x = self._scalars(1, 1)
                return 0.5 * s_res + 0.5 * reg_param * s_x

            alpha, _ = scalar_search_armijo(phi, cost, -g2, c1=1e-4, alpha0=1.0)      # :189-190 (derphi0 = grad . (-grad))
            self.n_feval.append(last[1])
            if alpha is None:
                print('line search failed at iteration %3d' % (k))
                break
            assert last[0] == alpha                                                 # the accepted step is the last one tried
            self.d_rec, trial = trial, self.d_rec                                   # :197  rec -= alpha grad  (the same float operation)
            self.d_tmp2 = trial
            if positivity or self.d_gt is not None:
                be.acc_zero(2, 1)
                be.clamp_err(self.d_rec, positivity, self.d_gt, slot=2)             # :200-201, :207
            err2 = self._scalars(0, 3)[2] if self.d_gt is not None else None
            convergence = np.sqrt(res2)                                             # :203
            rms_error[k] = convergence / self.norm_factor if self.d_gt is None else np.sqrt(err2) / self.norm_factor
            stop = self._semi_converged(k, rms_error, 1)                           # :209-213
            k += 1
        self.n_feval = np.array(self.n_feval, np.int64)
        return self._finish(rms_error, k)

    # ---- LASSO                                                                                        regularized.py:239-413
    def _backtrack_lasso(self, t, beta, res2, _lambda, xp):
        """regularized.py:317-332 around self.d_rec with gradient self.d_bp: -> (t, success); `xp` holds the last trial point
        soft(rec - t grad, t lambda) -- on success the ISTA update itself."""
        be = self.be
        g0 = 0.5 * res2
        while t > 1.e-16:
            be.acc_zero(0, 3)
            be.prox_l1_trial(xp, self.d_rec, self.d_bp, t, t * _lambda, slot=1)    # :321-322
            self.proj_mat.apply(xp, self.d_ax)
            be.residual_acc(None, self.d_ax, self.d_b, slot=0)                      # :324-325
            s_res, gGt, Gt2 = self._scalars(1, 2)
            g = 0.5 * s_res
            gp = g0 - gGt + (0.5 / t) * Gt2                                         # :326
            if g <= gp:
                return t, True
            t *= beta
        return t, False

    def _lasso_rms(self, res2, slot):
        if self.d_gt is None:
            return np.sqrt(res2) / self.norm_factor                                 # :280-282
        return np.sqrt(self._scalars(0, slot + 1)[slot]) / self.norm_factor         # :284

    def run_lasso_ista(self, niter=100, reg_param=1.0, alpha0=1.0, beta=0.5, make_plot=False):
        if make_plot:
            print(_NO_PLOT)
        be = self.be
        rms_error = np.zeros(niter, )
        self.step_size = np.zeros(niter, )
        xp = self._vol2()
        k, stop = 0, 0
        while k < niter and not stop:
            be.acc_zero(0, 1)
            self._residual_and_backprojection(negate=False)                         # :266-268  res = A rec - b ; grad = A^T res
            res2 = self._scalars(1, 0)[0]
            alpha, success = self._backtrack_lasso(alpha0, beta, res2, reg_param, xp)      # :271
            self.step_size[k] = alpha
            if not success:
                print('line search failed to converge')
                break
            self.d_rec, xp = xp, self.d_rec                                         # :278  the accepted trial IS the update
            self.d_tmp2 = xp
            if self.d_gt is not None:
                be.acc_zero(3, 1)
                be.clamp_err(self.d_rec, False, self.d_gt, slot=3)
            rms_error[k] = self._lasso_rms(res2, 3)
            stop = self._semi_converged(k, rms_error, 1)                           # :286-288
            k += 1
        rec, rms = self._finish(rms_error, k)
        return rec.reshape(self.vox_shape), rms                                     # :315

    def run_lasso_accelerated(self, niter=100, reg_param=1.0, alpha0=1.0, beta=0.5, make_plot=False):
        if make_plot:
            print(_NO_PLOT)
        be = self.be
        rms_error = np.zeros(niter, )
        xp = self._vol2()
        x_0, x_1 = self.d_tmp, be.zeros(self.n_vox)                                # :358-359  x_0 = x_1 = 0, whatever the warm start
        be.fill(x_0, 0.0)
        k, stop = 0, 0
        while k < niter and not stop:
            be.acc_zero(0, 1)
            self._residual_and_backprojection(negate=False)                         # :363-364
            res2 = self._scalars(1, 0)[0]
            alpha, success = self._backtrack_lasso(alpha0, beta, res2, reg_param, xp)      # :367 (around rec, not v; the trial is dropped)
            if not success:
                print('line search failed to converge')
                break
            be.acc_zero(3, 1)
            be.prox_l1_momentum(x_0, x_0, x_1, self.d_bp, (k - 2) / (k + 1), alpha, alpha * reg_param, gt=self.d_gt, slot=3)      # :374-375
            x_0, x_1 = x_1, x_0                                                     # :376-377
            self.d_rec = x_1
            rms_error[k] = self._lasso_rms(res2, 3)
            stop = self._semi_converged(k, rms_error, 1)                           # :385-389
            k += 1
        self.d_tmp = x_0
        return self._finish(rms_error, k)


def my_tikh_f(x, proj_mat, b, _lambda):
    """0.5 |A x - b|^2 + 0.5 lambda |x|^2 (regularized.py:416-422); proj_mat: any operator with .dot."""
    res = proj_mat.dot(np.ravel(x)) - np.ravel(b)
    return 0.5 * np.linalg.norm(res) ** 2 + 0.5 * _lambda * np.linalg.norm(x) ** 2


def my_tikh_fp(x, proj_mat, b, _lambda):
    """A^T (A x - b) + lambda x (regularized.py:425-430)."""
    res = proj_mat.dot(np.ravel(x)) - np.ravel(b)
    return proj_mat.T.dot(res) + _lambda * x


def soft_thresholding(x, _lambda, ctx=None):
    """x - l where x > l, x + l where x < -l, else 0.  numpy in -> numpy float32 out (same shape); DeviceArray in -> a new
    DeviceArray.  The device computes in float32: a float64 input comes back as FLOAT32, not as float32 values labelled
    float64 (the reference computes in the input's dtype)."""
    if isinstance(x, _lib.DeviceArray):
        c = x.ctx
        out = c.empty(x.shape)
        c.check(c.lib.tomo_vec_soft_threshold(c.handle, out.ptr, x.ptr, x.size, float(_lambda)))
        return out
    a = np.asarray(x)
    c = _tv._context(ctx)
    d = c.to_device(a.ravel())
    c.check(c.lib.tomo_vec_soft_threshold(c.handle, d.ptr, d.ptr, d.size, float(_lambda)))
    return d.download().reshape(a.shape)
