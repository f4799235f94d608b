/* gpk.h -- C ABI of libgpk.so: the MI355X (gfx950) implementation of the Gram-assembly + Gauss-Newton hot path of
 * yifanc96/NonLinPDEs-GPsolver.  The reference has no FFI of its own (it is pure Python on JAX); the boundary this
 * library replaces is the set of array-level operations its src/ modules hand to XLA.  Each entry point names the
 * reference call site(s) it stands in for (paths relative to the reference root).
 *
 * Conventions (all entry points):
 *   - return int: 0 ok; >0 LAPACK-style info (1-based index of the first non-positive pivot); <0 = -(hipError_t),
 *     text via gpk_last_error().  -9001 = invalid argument, -9002 = library built without a usable device.
 *   - every matrix/vector pointer is a DEVICE pointer owned by the caller unless the name says `host`; the library
 *     never frees or keeps them after the call.  Matrices are row-major double with a leading dimension in ELEMENTS;
 *     symmetric outputs are stored full.  Vector loads are 16-byte wide when pointer and leading dimension allow
 *     (even ld, 16-byte aligned base); any alignment is accepted (the matrix product then loads element by element; the
 *     substitution kernels keep their 16-byte loads at 8-byte alignment, which gfx950 global memory serves).  Operands are
 *     VIEWS: a routine writes its declared output region and nothing else, and triangular routines read only the lower
 *     triangle of L (tests/test_gpu_dense_views.py checks all three on unaligned views between canaries).
 *   - calls are asynchronous on the handle's stream; functions that return host scalars (info, loss, ratios)
 *     synchronise that stream.  One host thread per handle.  The library has NO process-wide mutable state (round 4): all
 *     state, including the development / tuning switches (gpk_debug.h: gpk_tune(handle, key, value), never called by the
 *     product path), lives in the handle, so handles of one process are independent of each other.
 *   - there is NO CPU fallback: without a gfx950 device gpk_create fails.
 */
#ifndef GPK_H
#define GPK_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpk_ctx* gpk_handle;

/* Gram layouts = the `eqn` strings of src/Gram_matrice.py:41,58,100,137 (Darcy yields two matrices: _U and _A). */
enum { GPK_LAYOUT_ELLIPTIC = 0, GPK_LAYOUT_BURGERS = 1, GPK_LAYOUT_EIKONAL = 2, GPK_LAYOUT_DARCY_U = 2, GPK_LAYOUT_DARCY_A = 3 };
/* kernel classes of src/kernels.py:8,91, and the Matern family nu = 5/2, 7/2, 9/2 ("Matern kernels"):
 *   kappa = exp(-t) theta_m(t) / theta_m(0),  nu = m + 1/2,  t = sqrt(2 nu) |((x1-y1)/rho_1, (x2-y2)/rho_2)|,  theta_m the reverse Bessel
 *   polynomial (nu = 5/2: (1 + t + t^2/3) exp(-t)).  host_kparams = {rho_1, rho_2}: BOTH are read, each finite and > 0, else -9001.
 * The Matern ids are served by the calls of the reference layouts -- gpk_assemble, gpk_assemble_test, gpk_extend, gpk_extend_functionals,
 * gpk_assemble_cross, for every layout -- and by nothing else: the 3-D, boundary-functional and operator calls return -9001 for them.
 * Ids 2..7 and every id above 10 but 16 are invalid everywhere (-9001).  nu = 3/2 is absent on purpose: that kernel is not C^4 at
 * coincident points, so the diagonal of a Laplacian block does not exist.
 * GPK_KERNEL_PERIODIC ("Periodic kernel"): the product over the two axes of
 *   kappa_k(d) = exp(-(2 p_k / w_k^2) sin^2(w_k d / 2)),  p_k = 2 / sigma_k^2,  w_k = 2 pi / L_k   on an axis with period L_k > 0,
 *   kappa_k(d) = exp(-p_k d^2 / 2)   (the anisotropic Gaussian factor)                                on an axis with L_k = 0,
 * so that every sample path, the posterior mean and all their derivatives have period L_k along axis k and that axis needs no boundary
 * points.  host_kparams = {sigma_1, sigma_2, L_1, L_2}: FOUR doubles are read; sigma_k finite and > 0, L_k finite and >= 0, not both
 * periods 0 (that kernel is GPK_KERNEL_ANISOTROPIC), else -9001 and nothing is launched.  Served by the same six calls as the Matern ids
 * (gpk_assemble, gpk_assemble_test, gpk_assemble_cross, gpk_assemble_prior, gpk_extend, gpk_extend_functionals) and by nothing else. */
enum { GPK_KERNEL_GAUSSIAN = 0, GPK_KERNEL_ANISOTROPIC = 1, GPK_KERNEL_MATERN52 = 8, GPK_KERNEL_MATERN72 = 9, GPK_KERNEL_MATERN92 = 10,
       GPK_KERNEL_PERIODIC = 16 };
/* nugget_type of src/PDEs.py:56,250,391 / src/InverseProblems.py:66 */
enum { GPK_NUGGET_NONE = 0, GPK_NUGGET_IDENTITY = 1, GPK_NUGGET_ADAPTIVE = 2 };
/* Gauss-Newton systems (measurement vector F(z) and Jacobian A(z) of each equation class) */
enum { GPK_GN_ELLIPTIC = 0, GPK_GN_BURGERS = 1, GPK_GN_EIKONAL = 2, GPK_GN_DARCY = 3, GPK_GN_ELLIPTIC_RELAXED = 4, GPK_GN_SEMILINEAR = 5, GPK_GN_MONGE_AMPERE = 6,
       GPK_GN_SEMILINEAR3D = 7, GPK_GN_QUASILINEAR = 9 };   /* (8 is not a system id: it stays invalid, -9001) */
/* GPK_GN_MONGE_AMPERE (no counterpart in the reference; DESIGN.md section K, "Fully nonlinear: Monge-Ampere"):
 *   det D^2 u = f, f > 0, convex branch, in the form  Delta u = sqrt((D u)^2 + (M u)^2 + 4 f),  D = d_11 - d_22,  M = 2 d_12
 * ((Delta u)^2 = (D u)^2 + (M u)^2 + 4 det D^2 u), on the rows of gpk_assemble_hess ([D u; M u; Delta u; u] per domain point, then the
 * boundary values), unknowns z = [v0 = u | v1 = D u | v2 = M u]:
 *   F(z) = [v1; v2; s; v0; g],  s = sqrt(v1^2 + v2^2 + 4 f),   A(z): 1 at (t, v1_t), (N_d + t, v2_t), (3 N_d + t, v0_t) and
 *   v1 / s, v2 / s at (2 N_d + t, v1_t / v2_t) -- the sparsity pattern of GPK_GN_EIKONAL, N = 4 N_d + N_b, n_z = 3 N_d.
 * gpk_gn_problem: rhs_f = f; p0, p1 are not read; nonlin must be 0 (-9001).  Where the radicand is negative s is NaN, and it
 * propagates through the step like every other NaN (loss and delta NaN): nothing on the device tests for it.
 * gpk_gn_structured_prepare and gpk_gn_gram_prepare refuse the system (-9001); gpk_posterior_prepare and gpk_log_evidence serve it. */
/* GPK_GN_SEMILINEAR (no counterpart in the reference; DESIGN.md section K, "Gradient-dependent nonlinearity"):
 *   -eps Delta u + N(u, grad u) = f,   N(u, p, q) = u (a1 p + a2 q) + b (p^2 + q^2) + c1 u + c3 u^3,   p = d_1 u, q = d_2 u,
 * on the rows of GPK_LAYOUT_EIKONAL ([d_1 u; d_2 u; Delta u; u] per domain point, then the boundary values), unknowns z = [v0 = u | v1 = p | v2 = q]:
 *   F(z) = [v1; v2; (N(v0, v1, v2) - f) / eps; v0; g],   A(z): 1 at (t, v1_t), (N_d + t, v2_t), (3 N_d + t, v0_t) and
 *   N_u / eps, N_p / eps, N_q / eps at (2 N_d + t, v0_t / v1_t / v2_t);  N_u = a1 p + a2 q + c1 + 3 c3 u^2, N_p = a1 u + 2 b p, N_q = a2 u + 2 b q.
 * gpk_gn_problem: p0 = eps (finite, not 0: -9001 otherwise), the five coefficients in gq_a1 .. gq_c3; nonlin must be 0 (-9001). */
/* GPK_GN_SEMILINEAR3D (no counterpart in the reference; DESIGN.md section K, "Gradient layout in three dimensions"):
 *   -psi[u] + N(u, grad u) = f,   N(u, g) = u (a1 g1 + a2 g2 + a3 g3) + b1 g1^2 + b2 g2^2 + b3 g3^2 + c1 u + c3 u^3,   g_k = d_k u,
 * on the rows of gpk_assemble_grad3d ([d_1 u; d_2 u; d_3 u; psi[u]; u] per domain point, then the boundary functionals), unknowns
 * z = [v0 = u | v1 | v2 | v3], n_z = 4 N_d, N = 5 N_d + N_b, one factor:
 *   F(z) = [v1; v2; v3; N(v0, v1, v2, v3) - f; v0; g],   A(z): 1 at (t, v1_t), (N_d + t, v2_t), (2 N_d + t, v3_t), (4 N_d + t, v0_t) and
 *   N_u, N_g1, N_g2, N_g3 at (3 N_d + t, v0_t / v1_t / v2_t / v3_t);  N_u = a . g + c1 + 3 c3 u^2,  N_gk = a_k u + 2 b_k g_k.
 * psi carries its own scale (eps Laplace, nu Laplace_x - d_t, ...: the op3 of gpk_assemble_grad3d), so the PDE row is not divided by anything.
 * gpk_gn_problem keeps its fields; the eight coefficients travel in doubles it already has:
 *   (a1, a2, a3) = (gq_a1, gq_a2, p0),   (b1, b2, b3) = (gq_b, p1, pen_lambda),   c1 = gq_c1,   c3 = gq_c3;
 * nonlin and p2 must be 0 (-9001).  gpk_gn_step runs it in the leading-zero layout with the unknowns in the order v1, v2, v3, v0: the
 * column at position pos then starts in row pos, one slope-1 staircase (the closed form of the elliptic system).  Served by gpk_gn_dims,
 * gpk_gn_worksize, gpk_gn_build(_rev), gpk_gn_measurement, gpk_gn_loss, gpk_gn_hessian_grad, gpk_gn_step, gpk_gn_direction, the line
 * search, gpk_posterior_prepare and gpk_log_evidence; gpk_gn_structured_prepare, gpk_gn_gram_prepare and gpk_mg_gn_step on more than one
 * GPU refuse it (-9001, named in gpk_last_error). */
/* GPK_GN_QUASILINEAR (no counterpart in the reference; DESIGN.md section K, "Quasilinear equations: the 2-jet layout"):
 *   a second-order equation in the plane whose second-order coefficients depend on grad u, solved for the Laplacian:  Delta u = G(x; v),
 * on the rows of gpk_assemble_jet2 ([d_1 u; d_2 u; D u; M u; Delta u; u] per domain point, D = d_11 - d_22, M = 2 d_12, then the boundary
 * values), unknowns z = [v0 = u | v1 = d_1 u | v2 = d_2 u | v3 = D u | v4 = M u], n_z = 5 N_d, N = 6 N_d + N_b, one factor:
 *   F(z) = [v1; v2; v3; v4; G(x; v); v0; g],   A(z): 1 at (t, v1_t), (N_d + t, v2_t), (2 N_d + t, v3_t), (3 N_d + t, v4_t), (5 N_d + t, v0_t)
 *   and dG/dv0 .. dG/dv4 at (4 N_d + t, v0_t / v1_t / v2_t / v3_t / v4_t) -- the v0 entry is written for every kind, also where it is 0.
 * The equation kind travels in `nonlin` as a GPK_QL_* id (read as such for this system only), its parameters in p0, p1, p2; rhs_f = f.
 * With p = v1, q = v2, g^2 = p^2 + q^2, W^2 = 1 + g^2, Q = v3 (p^2 - q^2) + 2 p q v4:
 *   GPK_QL_MEAN_CURVATURE  (p0 = kappa)          div(grad u / sqrt(1 + |grad u|^2)) = f + kappa u      G = (2 W^3 (f + kappa v0) + Q) / (1 + W^2)
 *   GPK_QL_P_LAPLACE       (p0 = m, p1 = delta)  div((delta^2 + |grad u|^2)^((m-2)/2) grad u) = f      G = (2 f (delta^2 + g^2)^((4-m)/2) - (m - 2) Q) / (2 delta^2 + m g^2)
 *   GPK_QL_GAUSS_CURVATURE (p0 = e)              det D^2 u = f (1 + |grad u|^2)^e, convex branch       G = sqrt(v3^2 + v4^2 + 4 f W^(2e))
 * (m = 2: Poisson's equation, a linear system; e = 0: GPK_GN_MONGE_AMPERE's root).  Both denominators are positive at every iterate and
 * the zero start is admissible; a negative radicand gives NaN, carried like any other.  An unknown kind, a parameter that is not finite,
 * m <= 0 or delta <= 0: -9001, nothing is launched.  gpk_gn_step runs it in the leading-zero layout with the unknowns in the order v1, v2,
 * v3, v4, v0: the column at position pos starts in row pos (dG/dv0 in the PDE row 4 N_d + t), one slope-1 staircase.  Served by
 * gpk_gn_dims, gpk_gn_worksize, gpk_gn_build(_rev), gpk_gn_measurement, gpk_gn_loss, gpk_gn_hessian_grad, gpk_gn_step, gpk_gn_direction,
 * the line search, gpk_posterior_prepare and gpk_log_evidence; gpk_gn_structured_prepare, gpk_gn_gram_prepare and gpk_mg_gn_step refuse
 * it (-9001, named in gpk_last_error). */
enum { GPK_QL_MEAN_CURVATURE = 0, GPK_QL_P_LAPLACE = 1, GPK_QL_GAUSS_CURVATURE = 2 };
/* Reaction term tau(u) of the elliptic systems, -psi[u] + tau(u) = f ("Reaction terms"); parameters p0, p1, p2:
 *   POWER  p0 pow(u, p1)              (alpha u^m: the reference's equation, and what a zeroed gpk_gn_problem means)
 *   EXP    p0 exp(p1 u)               SINH   p0 sinh(p1 u)              SIN   p0 sin(p1 u)
 *   CUBIC  u (p0 + u (p1 + p2 u))     (p0 u + p1 u^2 + p2 u^3: Allen-Cahn, Fisher-KPP, any cubic without a constant term) */
enum { GPK_NL_POWER = 0, GPK_NL_EXP = 1, GPK_NL_SINH = 2, GPK_NL_SIN = 3, GPK_NL_CUBIC = 4 };

/* ---- context, memory, stream ------------------------------------------------------------------------------ */
int gpk_create(int device, gpk_handle* out);
int gpk_destroy(gpk_handle h);
const char* gpk_last_error(gpk_handle h);
const char* gpk_version(void);
int gpk_set_stream(gpk_handle h, void* hip_stream);          /* NULL = the handle's own stream */
int gpk_synchronize(gpk_handle h);
int gpk_device_info(gpk_handle h, char* name, int name_len, int* compute_units, size_t* hbm_bytes, int* clock_khz);
int gpk_malloc(gpk_handle h, size_t bytes, void** dptr);
int gpk_free(gpk_handle h, void* dptr);
int gpk_memset(gpk_handle h, void* dptr, int value, size_t bytes);
int gpk_memcpy_h2d(gpk_handle h, void* dst, const void* host_src, size_t bytes);
int gpk_memcpy_d2h(gpk_handle h, void* host_dst, const void* src, size_t bytes);
int gpk_memcpy_d2d(gpk_handle h, void* dst, const void* src, size_t bytes);
int gpk_memcpy2d_h2d(gpk_handle h, void* dst, size_t dpitch, const void* host_src, size_t spitch, size_t width, size_t height);
int gpk_memcpy2d_d2h(gpk_handle h, void* host_dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height);
int gpk_memcpy2d_d2d(gpk_handle h, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height);

/* HIP-event stopwatch on the handle's stream (used by bench.py for per-kernel durations). */
int gpk_timer_start(gpk_handle h);
int gpk_timer_stop(gpk_handle h, double* host_ms);            /* synchronises */

/* Per-phase HIP-event timing inside gpk_gn_step, recorded on the handle's stream (bench.py's roofline leg):
 * host_ms4 = accumulated milliseconds of {TRSM phase, the SYRK launch, POTRF of H, TRSV + update} over *host_count steps. */
int gpk_prof_enable(gpk_handle h, int on);                    /* also resets the accumulators */
int gpk_prof_read(gpk_handle h, double* host_ms4, int* host_count);
/* gpk_gn_step forms Hb = S^T S and factors it in one pipelined phase (product by 512-column blocks on a GEMM stream, panel
 * chains on a second stream with a disjoint CU mask): host_ms4[1] is then the wall time of that whole phase and host_ms4[2]
 * is 0.  *host_pipelined = 1 if the last step ran pipelined; *host_syrk_launch_ms = accumulated duration of the SYRK launches
 * themselves (HIP events on the stream they ran on); *host_chain_cus = CUs of the chain partition. */
int gpk_prof_read_pipeline(gpk_handle h, int* host_pipelined, double* host_syrk_launch_ms, int* host_chain_cus);
/* Flops EXECUTED by the matrix-product launches issued while the per-phase timing was on, accumulated per phase from the K ranges
 * the launch logic gives its tiles (structural zeros of A(z), triangular operands and skipped upper tiles left out):
 * host_flops4 = {solve S = L^{-1}[A | F], updates inside the factorisation of Hb, the product Hb = S^T S, unused};
 * host_launches4 (may be NULL) = number of launches behind each figure.  The panel / substitution kernels are not counted. */
int gpk_prof_read_flops(gpk_handle h, double* host_flops4, long* host_launches4);
/* Duration of the Gram evaluator launch of the LAST gpk_assemble / gpk_assemble3d / gpk_assemble_bc / gpk_assemble_op / gpk_assemble_op3d / gpk_assemble_hess / gpk_assemble_jet2 / gpk_assemble_grad3d / gpk_assemble_disp / gpk_assemble_evo call issued while the per-phase timing was on (HIP events on the
 * handle's stream around that launch alone; the point packing kernel and the host-side set-up stay outside).  Synchronises. */
int gpk_prof_read_assembly(gpk_handle h, double* host_ms);

/* ---- Gram assembly: replaces Gram_matrix_assembly (src/Gram_matrice.py:11-187) plus the nugget of
 *      *.Gram_matrix (src/PDEs.py:56-73,250-269,391-409; src/InverseProblems.py:66-99) in one fused pass.
 *      kparams: Gaussian {sigma, unused}; anisotropic {sigma_t, sigma_x}; Matern {rho_1, rho_2}.  Xd (Nd,2), Xb (Nb,2) row-major.
 *      Theta: N x N, N = 2Nd+Nb (ELLIPTIC), 4Nd+Nb (BURGERS/EIKONAL/DARCY_U), 3Nd (DARCY_A).
 *      host_ratios[3]: adaptive trace ratios (unused entries 0). */
int gpk_assemble(gpk_handle h, int layout, int kernel, const double* host_kparams,
                 const double* Xd, int Nd, const double* Xb, int Nb,
                 double nugget, int nugget_type, double* Theta, int ld, double* host_ratios);
/* construct_Theta_test (src/Gram_matrice.py:190-289): out is Nt x N row-major.
 *      ld >= N (N as for gpk_assemble), else -9001 and nothing is written, as for NULL pointers and Nt <= 0. */
int gpk_assemble_test(gpk_handle h, int layout, int kernel, const double* host_kparams,
                      const double* Xt, int Nt, const double* Xd, int Nd, const double* Xb, int Nb,
                      double* out, int ld);
/* Theta_test @ coeff without materialising Theta_test: the matmul of *.extend_sol
 * (src/PDEs.py:208,350,505; src/InverseProblems.py:193,196).  coeff (N,), out (Nt,). */
int gpk_extend(gpk_handle h, int layout, int kernel, const double* host_kparams,
               const double* Xt, int Nt, const double* Xd, int Nd, const double* Xb, int Nb,
               const double* coeff, double* out);
/* Derivatives of the extension at test points, matrix-free: the rows of Theta_test with the row functional delta replaced by each
 * requested functional, times coeff = Theta^{-1} sol_vec (gpk_potrs, as for gpk_extend).  fmask: GPK_FN_* bits;
 * out is functional-major, row k (the k-th set bit of fmask, ascending) at out + k*ldo, ldo >= Nt; entries past Nt untouched.
 * The reduction order is fixed: a repeated call gives bit-identical output.  No reference call site (the reference has no derivative
 * extension; it is built from the kernel derivatives of src/kernels.py the Gram assembly already uses). */
/* row functionals of the extension (bit mask); for Burgers axis 1 is t, axis 2 is x */
enum { GPK_FN_VALUE = 1, GPK_FN_D1 = 2, GPK_FN_D2 = 4, GPK_FN_D2D2 = 8, GPK_FN_LAPLACIAN = 16 };
int gpk_extend_functionals(gpk_handle h, int layout, int kernel, const double* host_kparams,
                           const double* Xt, int Nt, const double* Xd, int Nd, const double* Xb, int Nb,
                           const double* coeff, int fmask, double* out, int ldo);
/* Pointwise PDE residual from rows of gpk_extend_functionals: out[t] = r(x_t), rhs[t] = f(x_t).  system = GPK_GN_*.
 *   fields_u (4 rows, ld ldu >= Nt): value, d1, d2, then d2d2 (BURGERS) or laplacian (all others);
 *   fields_a (3 rows, ld lda >= Nt): value, d1, d2 of the log-permeability a -- DARCY only, may be NULL otherwise;
 *   host_params3: the equation's Gauss-Newton parameters (alpha, m) / (alpha, nu) / (eps); not read for DARCY (may be NULL then).
 * The relations are those the Gauss-Newton systems eliminate (the sol_vec of src/PDEs.py:132-135,338-343,488-498; IP.py:176-186):
 *   ELLIPTIC(_RELAXED)  r = -Delta u + alpha u^m - f        (v1 = alpha v0^m - f, src/PDEs.py:132)
 *   BURGERS (t, x)      r = u_t + alpha u u_x - nu u_xx - f   (u_t = nu v3 + f - alpha v0 v2, src/PDEs.py:341)
 *   EIKONAL             r = |grad u|^2 - f^2 - eps Delta u    (v3 = -(f^2 - v1^2 - v2^2)/eps, src/PDEs.py:491)
 *   DARCY               r = -e^a (Delta u + grad a . grad u) - f   (v3 = -v1 w1 - v2 w2 - f e^{-w0}, src/InverseProblems.py:185) */
int gpk_pde_residual(gpk_handle h, int system, const double* host_params3, int Nt,
                     const double* fields_u, int ldu, const double* fields_a, int lda, const double* rhs, double* out);
/* The same for the elliptic equation with the reaction term tau = GPK_NL_* (nonlin) and host_params3 = (p0, p1, p2):
 *   r = -u3 + tau(u0) - f,   u0 = row 0 (value) and u3 = row 3 (Laplacian, or psi[u] under a domain operator) of fields_u (ld ldu >= Nt);
 * rows 1 and 2 are not read.  nonlin = GPK_NL_POWER gives the numbers of gpk_pde_residual(GPK_GN_ELLIPTIC).  nonlin outside the enum: -9001. */
int gpk_pde_residual_nl(gpk_handle h, int nonlin, const double* host_params3, int Nt,
                        const double* fields_u, int ldu, const double* rhs, double* out);
/* The same for the equation of GPK_GN_SEMILINEAR, host_gq5 = (a1, a2, b, c1, c3):
 *   r = -eps u3 + N(u0, u1, u2) - f,   rows 0..3 of fields (ld ldf >= Nt) = value, d1, d2, laplacian, as for gpk_pde_residual.
 * One fixed order of operations: a repeated call gives bit-identical output.  eps 0 or not finite, NULL pointers, Nt <= 0, ldf < Nt: -9001. */
int gpk_pde_residual_sl(gpk_handle h, double eps, const double* host_gq5, int Nt,
                        const double* fields, int ldf, const double* rhs, double* out);
/* The same for the Monge-Ampere equation: out[t] = d11 d22 - d12^2 - f, rows 0..2 of fields (ld ldf >= Nt) = d11, d12, d22 of the
 * extension (gpk_extend_functionals_hess).  One fixed order of operations ((d11 * d22 - d12 * d12) - f, no contraction): a repeated call
 * gives bit-identical output.  NULL pointers, Nt <= 0, ldf < Nt: -9001. */
int gpk_pde_residual_ma(gpk_handle h, int Nt, const double* fields, int ldf, const double* rhs, double* out);
/* The same for the equation of GPK_GN_SEMILINEAR3D, host_gq8 = (a1, a2, a3, b1, b2, b3, c1, c3):
 *   r = -psi_u + N(u0, u1, u2, u3) - f,   rows 0..3 of fields (ld ldf >= Nt) = value, d1, d2, d3 of the extension (gpk_extend_functionals_grad3d),
 * psi_u (Nt) = psi_t[u] at the test points, which the caller has combined from the extension rows.  One fixed order of operations
 * ((N - psi_u) - f with the N of the Gauss-Newton build, no contraction): a repeated call gives bit-identical output.  NULL pointers, Nt <= 0,
 * ldf < Nt: -9001. */
int gpk_pde_residual_sl3d(gpk_handle h, const double* host_gq8, int Nt, const double* fields, int ldf, const double* psi_u,
                          const double* rhs, double* out);
/* The same for the equations of GPK_GN_QUASILINEAR in their DIVERGENCE / DETERMINANT form (not Delta u - G), kind = GPK_QL_*,
 * host_params3 = (p0, p1, p2) as in gpk_gn_problem; rows 0..5 of fields (ld ldf >= Nt) = value, d1, d2, d11, d12, d22 of the extension
 * (gpk_extend_functionals_jet2).  With T = u1^2 u11 + 2 u1 u2 u12 + u2^2 u22, g^2 = u1^2 + u2^2:
 *   MEAN_CURVATURE   ((1 + g^2) Delta u - T) / (1 + g^2)^(3/2) - (f + kappa u)
 *   P_LAPLACE        (delta^2 + g^2)^((m-4)/2) ((delta^2 + g^2) Delta u + (m - 2) T) - f
 *   GAUSS_CURVATURE  (u11 u22 - u12^2) - f (1 + g^2)^e
 * One fixed order of operations, no contraction: a repeated call gives bit-identical output.  A kind or parameters the system refuses,
 * NULL pointers, Nt <= 0, ldf < Nt: -9001. */
int gpk_pde_residual_ql(gpk_handle h, int kind, const double* host_params3, int Nt, const double* fields, int ldf, const double* rhs,
                        double* out);
/* ---- three space dimensions: the nonlinear elliptic equation on a box in R^3 (no reference call site: the reference's assembly is written
 *      for (n,2) points; the method is the same -- DESIGN.md section K, "Three dimensions").  Points are (n,3) row-major, contiguous.
 *      host_kparams: Gaussian {sigma} (p_k = 1/sigma^2 on all three axes); anisotropic {sigma_1, sigma_2, sigma_3} (p_k = 2/sigma_k^2).
 *      Layout ELLIPTIC3D: block 0 = Laplacian on the Nd domain points, block 1 = delta on the Nd+Nb domain+boundary points; Theta is
 *      N x N, N = 2Nd+Nb -- the same shape as GPK_LAYOUT_ELLIPTIC, so gpk_potrf, the GPK_GN_ELLIPTIC system and gpk_pde_residual apply unchanged.
 *      host_ratio (one double, may be NULL): trace(block 0) / trace(block 1) = Nd <Lap,Lap>(0) / (Nd+Nb), written for every nugget type.
 *      Any alignment of Theta / ld is accepted (16-byte stores when base, ld, Nd and Nb allow; 8-byte stores otherwise); the launch is
 *      timed like gpk_assemble's when the per-phase timing is on (gpk_prof_read_assembly). */
int gpk_assemble3d(gpk_handle h, int kernel, const double* host_kparams,
                   const double* Xd, int Nd, const double* Xb, int Nb,
                   double nugget, int nugget_type, double* Theta, int ld, double* host_ratio);
/* Value and derivatives of the 3-D extension at test points Xt (Nt,3), matrix-free, as gpk_extend_functionals: coeff (2Nd+Nb) =
 * Theta^{-1} sol_vec.  fmask: a non-empty subset of GPK_FN_VALUE, GPK_FN_D1, GPK_FN_D2, GPK_FN_D3, GPK_FN_LAPLACIAN (anything else,
 * GPK_FN_D2D2 included: -9001); fmask == GPK_FN_VALUE is the plain extension.  out is functional-major, row k (the k-th set bit of
 * fmask, ascending: value, d1, d2, laplacian, d3) at out + k*ldo, ldo >= Nt; entries past Nt untouched.  Fixed reduction order: a
 * repeated call gives bit-identical output. */
#define GPK_FN_D3 32          /* d/dx3: 3-D calls only (bit 5, next to the GPK_FN_* bits above) */
int gpk_extend_functionals3d(gpk_handle h, int kernel, const double* host_kparams,
                             const double* Xt, int Nt, const double* Xd, int Nd, const double* Xb, int Nb,
                             const double* coeff, int fmask, double* out, int ldo);
/* ---- boundary functionals for the 2-D elliptic layout: Neumann, Robin and mixed conditions (no reference call site: the reference puts
 *      delta on every boundary row, Dirichlet data only; the method is the same -- DESIGN.md section K, "Boundary functionals").
 *      Layout as GPK_LAYOUT_ELLIPTIC -- block 0 = Laplacian on the Nd domain points, block 1 on the Nd+Nb domain+boundary points,
 *      N = 2Nd+Nb -- but boundary point b carries phi_b = c0 delta + c1 d/dx1 + c2 d/dx2 instead of delta (domain points keep delta):
 *      Dirichlet (1,0,0), Neumann (0,n1,n2), Robin (beta,n1,n2) with n the outward unit normal.  gpk_potrf, the GPK_GN_ELLIPTIC system
 *      (bdy_g = the prescribed values of phi_b u), gpk_potrs and gpk_pde_residual apply unchanged.
 *      bc: device pointer, (Nb,3) row-major doubles (c0, c1, c2) per boundary point; NULL = all (1,0,0), the entries of gpk_assemble.
 *      host_kparams, Xd, Xb as gpk_assemble.  host_ratio (one double, may be NULL): trace(block 0) / trace(block 1) =
 *      Nd (3 p1^2 + 2 p1 p2 + 3 p2^2) / (Nd + sum_b (c0_b^2 + p1 c1_b^2 + p2 c2_b^2)), written for every nugget type; the boundary sum is
 *      taken on the host in index order (bc != NULL: one small device-to-host copy, synchronises).
 *      Any alignment of Theta / ld is accepted (16-byte stores when base, ld, Nd and Nb allow; 8-byte stores otherwise; nothing outside
 *      the N x N view is written); the launch is timed like gpk_assemble's when the per-phase timing is on (gpk_prof_read_assembly). */
int gpk_assemble_bc(gpk_handle h, int kernel, const double* host_kparams, const double* Xd, int Nd, const double* Xb, int Nb,
                    const double* bc, double nugget, int nugget_type, double* Theta, int ld, double* host_ratio);
/* Value and derivatives of the extension under boundary functionals at test points Xt (Nt,2), matrix-free, as gpk_extend_functionals:
 * coeff (2Nd+Nb) = Theta^{-1} sol_vec with the Theta of gpk_assemble_bc for the same bc.  fmask: a non-empty subset of the GPK_FN_* bits
 * (anything else: -9001); out is functional-major, row k (the k-th set bit of fmask, ascending) at out + k*ldo, ldo >= Nt; entries
 * past Nt untouched.  Fixed reduction order: a repeated call gives bit-identical output.  No reference call site. */
int gpk_extend_functionals_bc(gpk_handle h, int kernel, const double* host_kparams, const double* Xt, int Nt,
                              const double* Xd, int Nd, const double* Xb, int Nb, const double* bc,
                              const double* coeff, int fmask, double* out, int ldo);
/* ---- Variable-coefficient operator on the domain points of the 2-D elliptic layout ("Variable-coefficient operator"):
 *      -psi[u] + alpha u^m = f with psi_i = c0 delta + b1 d_1 + b2 d_2 + a11 d_1 d_1 + a12 d_1 d_2 + a22 d_2 d_2 at domain point i.
 *      No reference call site (the reference solves -Laplace(u) + alpha u^m = f only).
 *      op (Nd,6) row-major on the device: row i = (c0, b1, b2, a11, a12, a22) of psi_i; a12 multiplies d_1 d_2 ONCE (a symmetric
 *      tensor A enters as a12 = 2 A12).  op == NULL: the Laplacian (0,0,0,1,0,1) at every domain point.  bc (Nb,3) / NULL: the
 *      boundary functionals of gpk_assemble_bc.  Layout as GPK_LAYOUT_ELLIPTIC: block 0 = psi on the Nd domain points, block 1 = delta
 *      on the domain points and phi_b on the boundary points, N = 2Nd+Nb, Theta N x N with leading dimension ld >= N -- so gpk_potrf,
 *      the GPK_GN_ELLIPTIC system and gpk_pde_residual apply unchanged (psi[u] takes the place of the Laplacian).
 *      Nugget as gpk_assemble's.  host_ratio (one double, may be NULL): trace(block 0) / trace(block 1) with the values at d = 0,
 *        <psi,psi> = c0^2 + p1 b1^2 + p2 b2^2 + 3 p1^2 a11^2 + 3 p2^2 a22^2 + p1 p2 (a12^2 + 2 a11 a22) - 2 c0 (p1 a11 + p2 a22),
 *        <phi,phi> = c0^2 + p1 c1^2 + p2 c2^2 (1 at a domain point),
 *      written for every nugget type; both point sums are taken on the host in index order (op / bc != NULL: one small device-to-host
 *      copy each, synchronises).  Any alignment of Theta / ld is accepted (16-byte stores when base, ld, Nd and Nb allow; 8-byte stores
 *      otherwise; nothing outside the N x N view is written); the launch is timed like gpk_assemble's when the per-phase timing is on
 *      (gpk_prof_read_assembly). */
int gpk_assemble_op(gpk_handle h, int kernel, const double* host_kparams, const double* Xd, int Nd, const double* Xb, int Nb,
                    const double* op, const double* bc, double nugget, int nugget_type, double* Theta, int ld, double* host_ratio);
/* The six monomial derivatives of the extension under op / bc at test points Xt (Nt,2), matrix-free: coeff (2Nd+Nb) = Theta^{-1} sol_vec
 * with the Theta of gpk_assemble_op for the same op and bc.  fmask: a non-empty subset of the GPK_OPFN_* bits below (anything else:
 * -9001); out is functional-major, row k (the k-th set bit of fmask, ascending) at out + k*ldo, ldo >= Nt; entries past Nt untouched.
 * Fixed reduction order: a repeated call gives bit-identical output, and a row has the same bits whichever other rows are requested.
 * psi_t[u] at a test point is a combination of the rows, formed by the caller. */
#define GPK_OPFN_VALUE 1      /* u */
#define GPK_OPFN_D1    2      /* du/dx1 */
#define GPK_OPFN_D2    4      /* du/dx2 */
#define GPK_OPFN_D11   8      /* d^2u/dx1^2 */
#define GPK_OPFN_D12  16      /* d^2u/dx1dx2 */
#define GPK_OPFN_D22  32      /* d^2u/dx2^2 */
int gpk_extend_functionals_op(gpk_handle h, int kernel, const double* host_kparams, const double* Xt, int Nt,
                              const double* Xd, int Nd, const double* Xb, int Nb, const double* op, const double* bc,
                              const double* coeff, int fmask, double* out, int ldo);
/* ---- Hessian layout: the second derivatives of u at the domain points as separate row blocks ("Fully nonlinear:
 *      Monge-Ampere").  No reference call site.  With D = d_11 - d_22, M = 2 d_12: block 0 = D, block 1 = M, block 2 = Laplacian, each
 *      on the Nd domain points; block 3 = delta on the Nd+Nb domain and boundary points.  N = 4Nd+Nb, Theta N x N, ld >= N: gpk_potrf,
 *      gpk_potrs and the GPK_GN_MONGE_AMPERE system apply to it.  Kernels: Gaussian and anisotropic Gaussian (Matern ids: -9001).
 *      host_kparams, Xd, Xb as gpk_assemble.  Nugget as gpk_assemble's for GPK_LAYOUT_EIKONAL: adaptive = nugget * trace ratio on each
 *      derivative block, nugget on block 3.  host_ratios3 (three doubles, may be NULL) = trace(block k) / trace(block 3), k = 0, 1, 2,
 *      with the values at d = 0
 *        <D,D> = 3 p1^2 - 2 p1 p2 + 3 p2^2,   <M,M> = 4 p1 p2,   <Lap,Lap> = 3 p1^2 + 2 p1 p2 + 3 p2^2,   <delta,delta> = 1,
 *      written for every nugget type.  Any alignment of Theta / ld is accepted (16-byte stores when base, ld, Nd and Nb allow; 8-byte
 *      stores otherwise, with the same values; nothing outside the N x N view is written); the launch is timed like gpk_assemble's
 *      when the per-phase timing is on (gpk_prof_read_assembly).  Bad arguments: -9001, named in gpk_last_error. */
int gpk_assemble_hess(gpk_handle h, int kernel, const double* host_kparams, const double* Xd, int Nd, const double* Xb, int Nb,
                      double nugget, int nugget_type, double* Theta, int ld, double* host_ratios3);
/* The six monomial derivatives of the extension on the Hessian layout at test points Xt (Nt,2), matrix-free: coeff (4Nd+Nb) =
 * Theta^{-1} sol_vec with the Theta of gpk_assemble_hess.  fmask: a non-empty subset of the GPK_OPFN_* bits (anything else: -9001); out
 * is functional-major, row k (the k-th set bit of fmask, ascending) at out + k*ldo, ldo >= Nt; entries past Nt untouched.  Fixed
 * reduction order: a repeated call gives bit-identical output, and a row has the same bits whichever other rows are requested. */
int gpk_extend_functionals_hess(gpk_handle h, int kernel, const double* host_kparams, const double* Xt, int Nt,
                                const double* Xd, int Nd, const double* Xb, int Nb,
                                const double* coeff, int fmask, double* out, int ldo);
/* ---- 2-jet layout: the first AND second derivatives of u at the domain points as separate row blocks (DESIGN.md section K,
 *      "Quasilinear equations: the 2-jet layout").  No reference call site.  Block 0 = d_1, block 1 = d_2, block 2 = D = d_11 - d_22,
 *      block 3 = M = 2 d_12, block 4 = Laplacian, each on the Nd domain points; block 5 = delta on the Nd+Nb domain and boundary points.
 *      N = 6Nd+Nb, Theta N x N, ld >= N: gpk_potrf, gpk_potrs and the GPK_GN_QUASILINEAR system apply to it.  Blocks 2..5 hold the
 *      entries of gpk_assemble_hess for the same points.  Theta is symmetric to the bit.  Kernels: Gaussian and anisotropic Gaussian
 *      (any other id: -9001).  host_kparams, Xd, Xb as gpk_assemble.  Nugget as gpk_assemble_hess: adaptive = nugget * trace(block k) /
 *      trace(block 5) on the blocks 0..4, nugget on block 5.  host_ratios5 (five doubles, may be NULL) = those ratios, with the values at d = 0
 *        <d_k,d_k> = p_k,   <D,D> = 3 p1^2 - 2 p1 p2 + 3 p2^2,   <M,M> = 4 p1 p2,   <Lap,Lap> = 3 p1^2 + 2 p1 p2 + 3 p2^2,   <delta,delta> = 1,
 *      written for every nugget type.  Any alignment of Theta / ld is accepted (16-byte stores when base, ld, Nd and Nb allow; 8-byte
 *      stores otherwise, with the same values; nothing outside the N x N view is written); the launch is timed like gpk_assemble's
 *      when the per-phase timing is on (gpk_prof_read_assembly).  Bad arguments: -9001, named in gpk_last_error. */
int gpk_assemble_jet2(gpk_handle h, int kernel, const double* host_kparams, const double* Xd, int Nd, const double* Xb, int Nb,
                      double nugget, int nugget_type, double* Theta, int ld, double* host_ratios5);
/* The six monomial derivatives of the extension on the 2-jet layout at test points Xt (Nt,2), matrix-free: coeff (6Nd+Nb) =
 * Theta^{-1} sol_vec with the Theta of gpk_assemble_jet2.  fmask, out, ldo and the contract (fixed reduction order, a row's bits do not
 * depend on the other rows requested) as gpk_extend_functionals_hess. */
int gpk_extend_functionals_jet2(gpk_handle h, int kernel, const double* host_kparams, const double* Xt, int Nt,
                                const double* Xd, int Nd, const double* Xb, int Nb,
                                const double* coeff, int fmask, double* out, int ldo);
/* ---- Dispersive layout: the Burgers layout with the third space derivative in place of the second ("Dispersive
 *      equations: the third-order layout"), for u_t + alpha u u_x + delta u_xxx = f.  No reference call site.  Points are (t, x) rows: axis 1
 *      is time, axis 2 is space, as for GPK_LAYOUT_BURGERS.  Block 0 = d_t, block 1 = d_x, block 2 = d_x^3, each on the Nd domain points;
 *      block 3 = delta on the Nd+Nb domain and boundary points.  N = 4Nd+Nb, Theta N x N, ld >= N: gpk_potrf, gpk_potrs, the
 *      GPK_GN_BURGERS system with p1 = -delta, gpk_log_evidence and gpk_pde_residual(GPK_GN_BURGERS) with u_xxx in the fourth row apply
 *      to it.  Theta is symmetric to the bit.  Kernels: Gaussian and anisotropic Gaussian (any other id: -9001).  host_kparams, Xd, Xb as
 *      gpk_assemble.  Nugget as gpk_assemble_hess: adaptive = nugget * trace(block k) / trace(block 3) on the blocks 0..2, nugget on
 *      block 3.  host_ratios3 (three doubles, may be NULL) = those ratios, with the values at d = 0
 *        <d_t,d_t> = p1,   <d_x,d_x> = p2,   <d_x^3,d_x^3> = 15 p2^3,   <delta,delta> = 1,
 *      written for every nugget type.  Any alignment of Theta / ld is accepted (16-byte stores when base, ld, Nd and Nb allow; 8-byte
 *      stores otherwise, with the same values; nothing outside the N x N view is written); the launch is timed like gpk_assemble's
 *      when the per-phase timing is on (gpk_prof_read_assembly).  Bad arguments: -9001, named in gpk_last_error. */
int gpk_assemble_disp(gpk_handle h, int kernel, const double* host_kparams, const double* Xd, int Nd, const double* Xb, int Nb,
                      double nugget, int nugget_type, double* Theta, int ld, double* host_ratios3);
/* Value and derivatives of the extension on the dispersive layout at test points Xt (Nt,2), matrix-free: coeff (4Nd+Nb) =
 * Theta^{-1} sol_vec with the Theta of gpk_assemble_disp.  fmask: a non-empty subset of GPK_FN_VALUE, GPK_FN_D1 (u_t), GPK_FN_D2 (u_x),
 * GPK_FN_D2D2 (u_xx) and GPK_FN_D2D2D2 (u_xxx) (anything else, GPK_FN_LAPLACIAN and GPK_FN_D3 included: -9001); out is functional-major,
 * row k (the k-th set bit of fmask, ascending) at out + k*ldo, ldo >= Nt; entries past Nt untouched.  Fixed reduction order (wave
 * shuffles, then LDS, no atomics): a repeated call gives bit-identical output, and a row has the same bits whichever other rows are
 * requested. */
#define GPK_FN_D2D2D2 64      /* d^3/dx2^3: gpk_extend_functionals_disp only (bit 6, after GPK_FN_LAPLACIAN and GPK_FN_D3) */
int gpk_extend_functionals_disp(gpk_handle h, int kernel, const double* host_kparams, const double* Xt, int Nt,
                                const double* Xd, int Nd, const double* Xb, int Nb,
                                const double* coeff, int fmask, double* out, int ldo);
/* ---- Evolution layout: the Burgers layout with a general spatial operator in place of the second space derivative (DESIGN.md section K,
 *      "Evolution equations: the general spatial operator"), for u_t + alpha u u_x + Q[u] = f with
 *        Q = c2 d_x^2 + c3 d_x^3 + c4 d_x^4 + c5 d_x^5,   host_c4 = {c2, c3, c4, c5} (finite, not all zero: otherwise -9001)
 *      -- Kuramoto-Sivashinsky (c2 = c4 = 1), Kawahara (c3, c5), KdV-Burgers (c2 = -nu, c3 = delta), Benney-Lin (all four).  No reference
 *      call site.  Points are (t, x) rows.  Block 0 = d_t, block 1 = d_x, block 2 = Q, each on the Nd domain points; block 3 = delta on
 *      the Nd domain points followed by c0 delta + c1 d_t + c2 d_x on the Nb boundary points, with (c0, c1, c2) = row b of bc (device,
 *      (Nb,3) row-major, the format of gpk_assemble_bc; NULL = delta everywhere).  N = 4Nd+Nb, Theta N x N, ld >= N: gpk_potrf, gpk_potrs,
 *      the GPK_GN_BURGERS system with p1 = -1, gpk_log_evidence and gpk_pde_residual(GPK_GN_BURGERS) with Q[u] in the fourth row apply to
 *      it.  Theta is symmetric to the bit.  Kernels: Gaussian and anisotropic Gaussian (any other id: -9001).  host_kparams, Xd, Xb as
 *      gpk_assemble.  Nugget as gpk_assemble_disp: adaptive = nugget * trace(block k) / trace(block 3) on the blocks 0..2, nugget on
 *      block 3.  host_ratios3 (three doubles, may be NULL) = those ratios, with the values at d = 0
 *        <d_t,d_t> = p1,   <d_x,d_x> = p2,   <delta,delta> = 1,   <B_b,B_b> = c0^2 + p1 c1^2 + p2 c2^2,
 *        <Q,Q> = 3 c2^2 p2^2 + 15 c3^2 p2^3 + 105 c4^2 p2^4 + 945 c5^2 p2^5 - 30 c2 c4 p2^3 - 210 c3 c5 p2^4,
 *      written for every nugget type (bc != NULL: the call reads bc back and synchronises the stream).  Any alignment of Theta / ld is
 *      accepted (16-byte stores when base, ld, Nd and Nb allow; 8-byte stores otherwise, with the same values; nothing outside the
 *      N x N view is written); the launch is timed like gpk_assemble's when the per-phase timing is on (gpk_prof_read_assembly).  Bad
 *      arguments: -9001, named in gpk_last_error, before any launch. */
int gpk_assemble_evo(gpk_handle h, int kernel, const double* host_kparams, const double* host_c4 /* c2..c5 */,
                     const double* Xd, int Nd, const double* Xb, int Nb, const double* bc /* (Nb,3) device, NULL = delta */,
                     double nugget, int nugget_type, double* Theta, int ld, double* host_ratios3);
/* Value and derivatives of the extension on the evolution layout at test points Xt (Nt,2), matrix-free: coeff (4Nd+Nb) =
 * Theta^{-1} sol_vec with the Theta of gpk_assemble_evo (the same host_c4 and bc).  fmask: a non-empty subset of GPK_FN_VALUE, GPK_FN_D1
 * (u_t), GPK_FN_D2 (u_x), GPK_FN_D2D2 (u_xx) and GPK_FN_Q (Q[u]) (anything else, GPK_FN_D2D2D2 included: -9001); out is functional-major,
 * row k (the k-th set bit of fmask, ascending) at out + k*ldo, ldo >= Nt; entries past Nt untouched.  Fixed reduction order (wave
 * shuffles, then LDS, no atomics): a repeated call gives bit-identical output. */
#define GPK_FN_Q 128          /* Q[u] = sum_k c_k d^k/dx2^k: gpk_extend_functionals_evo only (bit 7, after GPK_FN_D2D2D2) */
int gpk_extend_functionals_evo(gpk_handle h, int kernel, const double* host_kparams, const double* host_c4,
                               const double* Xt, int Nt, const double* Xd, int Nd, const double* Xb, int Nb, const double* bc,
                               const double* coeff, int fmask, double* out, int ldo);
/* ---- Operator and boundary functionals in three dimensions ("Operator and boundary functionals in three dimensions"):
 *      -psi[u] + alpha u^m = f on a box in R^3 with psi_i = c0 delta + sum_k b_k d_k + sum_{k<=l} a_kl d_k d_l at domain point i -- 3-D
 *      advection-diffusion-reaction, and with axis 3 as time psi = nu (d_1 d_1 + d_2 d_2) - d_3: u_t - nu Laplace_x u + alpha u^m = f in two
 *      space dimensions by space-time collocation.  No reference call site.
 *      op3 (Nd,10) row-major on the device: row i = (c0, b1, b2, b3, a11, a12, a13, a22, a23, a33) of psi_i; a mixed coefficient
 *      multiplies its mixed derivative ONCE (a symmetric tensor A enters as a12 = 2 A12).  op3 == NULL: the Laplacian
 *      (0,0,0,0,1,0,0,1,0,1) at every domain point.  bc3 (Nb,4) row-major on the device: row b = (c0, c1, c2, c3) of
 *      phi_b = c0 delta + c1 d_1 + c2 d_2 + c3 d_3 (Dirichlet (1,0,0,0), Neumann (0,n), Robin (beta,n)); bc3 == NULL: (1,0,0,0).
 *      Points (n,3) row-major, host_kparams and precisions as gpk_assemble3d.  Layout as ELLIPTIC3D: block 0 = psi on the Nd domain
 *      points, block 1 = delta on the domain points and phi_b on the boundary points, N = 2Nd+Nb, Theta N x N with leading dimension
 *      ld >= N -- so gpk_potrf, the GPK_GN_ELLIPTIC system, gpk_potrs and gpk_pde_residual apply unchanged (psi[u] takes the place of
 *      the Laplacian).  Nugget as gpk_assemble's.  host_ratio (one double, may be NULL): trace(block 0) / trace(block 1) with
 *        <psi,psi> = c0^2 + sum_k p_k b_k^2 + 3 sum_k p_k^2 a_kk^2 + sum_{k<l} p_k p_l (a_kl^2 + 2 a_kk a_ll) - 2 c0 sum_k p_k a_kk,
 *        <phi,phi> = c0^2 + sum_k p_k c_k^2 (1 at a domain point)
 *      at d = 0, written for every nugget type; both point sums are taken on the host in index order (op3 / bc3 != NULL: one small
 *      device-to-host copy each, synchronises).  Any alignment of Theta / ld is accepted (16-byte stores when base, ld, Nd and Nb
 *      allow; 8-byte stores otherwise, with the same values; nothing outside the N x N view is written); the launch is timed like
 *      gpk_assemble's when the per-phase timing is on (gpk_prof_read_assembly).  Bad arguments: -9001, named in gpk_last_error. */
int gpk_assemble_op3d(gpk_handle h, int kernel, const double* host_kparams, const double* Xd, int Nd, const double* Xb, int Nb,
                      const double* op3, const double* bc3, double nugget, int nugget_type, double* Theta, int ld, double* host_ratio);
/* The ten monomial derivatives of the extension under op3 / bc3 at test points Xt (Nt,3), matrix-free: coeff (2Nd+Nb) = Theta^{-1} sol_vec
 * with the Theta of gpk_assemble_op3d for the same op3 and bc3.  fmask: a non-empty subset of the GPK_OP3FN_* bits below, bit j =
 * monomial j of op3 (anything else: -9001); out is functional-major, row k (the k-th set bit of fmask, ascending) at out + k*ldo,
 * ldo >= Nt; entries past Nt untouched.  Three kernel instantiations serve every mask (value; value and gradient; all ten), the
 * smallest that contains the request.  Fixed reduction order: a repeated call gives bit-identical output, and a row has the same bits
 * whichever other rows are requested.  psi_t[u] at a test point is a combination of the rows, formed by the caller. */
#define GPK_OP3FN_VALUE 1     /* u */
#define GPK_OP3FN_D1    2     /* du/dx1 */
#define GPK_OP3FN_D2    4     /* du/dx2 */
#define GPK_OP3FN_D3    8     /* du/dx3 */
#define GPK_OP3FN_D11  16     /* d^2u/dx1^2 */
#define GPK_OP3FN_D12  32     /* d^2u/dx1dx2 */
#define GPK_OP3FN_D13  64     /* d^2u/dx1dx3 */
#define GPK_OP3FN_D22 128     /* d^2u/dx2^2 */
#define GPK_OP3FN_D23 256     /* d^2u/dx2dx3 */
#define GPK_OP3FN_D33 512     /* d^2u/dx3^2 */
int gpk_extend_functionals_op3d(gpk_handle h, int kernel, const double* host_kparams, const double* Xt, int Nt,
                                const double* Xd, int Nd, const double* Xb, int Nb, const double* op3, const double* bc3,
                                const double* coeff, int fmask, double* out, int ldo);
/* ---- Gradient layout in three dimensions ("Gradient layout in three dimensions"): the rows an equation that is
 *      nonlinear in grad u needs, -psi[u] + N(u, grad u) = f on a box in R^3 or, with axis 3 as time, in two space dimensions.  No
 *      reference call site.  Blocks 0, 1, 2 = d_1, d_2, d_3 on the Nd domain points, block 3 = psi_i on the domain points, block 4 = delta
 *      on the domain points followed by phi_b on the Nb boundary points: N = 5Nd+Nb, Theta N x N with leading dimension ld >= N.  op3
 *      (Nd,10) / NULL, bc3 (Nb,4) / NULL, points, host_kparams and precisions exactly as gpk_assemble_op3d (whose blocks 0, 1 are the
 *      blocks 3, 4 here).  Kernels: Gaussian and anisotropic Gaussian (any other id: -9001).  gpk_potrf, gpk_potrs and the
 *      GPK_GN_SEMILINEAR3D system apply to it.  Nugget as gpk_assemble_hess: adaptive = nugget * trace(block k) / trace(block 4) on the
 *      blocks k = 0..3, nugget on block 4.  host_ratios4 (four doubles, may be NULL) = those ratios with the values at d = 0
 *        <d_k, d_k> = p_k,   <psi, psi> and <phi, phi> as gpk_assemble_op3d,
 *      written for every nugget type; the point sums are taken on the host in index order (op3 / bc3 != NULL: one small device-to-host
 *      copy each, synchronises).  Any alignment of Theta / ld is accepted (16-byte stores when base, ld, Nd and Nb allow; 8-byte stores
 *      otherwise, with the same values; nothing outside the N x N view is written); the launch is timed like gpk_assemble's when the
 *      per-phase timing is on (gpk_prof_read_assembly).  Bad arguments: -9001, named in gpk_last_error. */
int gpk_assemble_grad3d(gpk_handle h, int kernel, const double* host_kparams, const double* Xd, int Nd, const double* Xb, int Nb,
                        const double* op3, const double* bc3, double nugget, int nugget_type, double* Theta, int ld, double* host_ratios4);
/* The ten monomial derivatives of the extension on the gradient layout at test points Xt (Nt,3), matrix-free: coeff (5Nd+Nb) =
 * Theta^{-1} sol_vec with the Theta of gpk_assemble_grad3d for the same op3 and bc3.  fmask, out, ldo and the guarantees (fixed reduction
 * order, a row has the same bits whichever other rows are requested) as gpk_extend_functionals_op3d. */
int gpk_extend_functionals_grad3d(gpk_handle h, int kernel, const double* host_kparams, const double* Xt, int Nt,
                                  const double* Xd, int Nd, const double* Xb, int Nb, const double* op3, const double* bc3,
                                  const double* coeff, int fmask, double* out, int ldo);
/* solver_GP.collocation_pts_err / get_test_error (src/solver.py:169-178, 185-194): err_all[i] = |truth[i] - approx[i]| (device, may be
 * NULL), *host_max = max_i err_all[i], *host_l2 = sqrt(sum_i err_all[i]^2 / n) -- the reference's "L2 error".  All inputs on the
 * device (the extension already is); one pass, fixed summation order.  Synchronises. */
int gpk_error_metrics(gpk_handle h, int n, const double* truth, const double* approx, double* err_all,
                      double* host_max, double* host_l2);

/* ---- dense fp64 linear algebra on the MFMA units --------------------------------------------------------- */
/* jnp.linalg.cholesky (src/PDEs.py:77,273,413; src/InverseProblems.py:102-103): lower factor in place.  Only the lower
 * triangle of A is read.  The strict upper triangle of the n x n view is UNSPECIFIED on return (the blocked updates write
 * whole tiles above the diagonal of the diagonal blocks; nothing ever reads them -- gpk_tril zeroes it); nothing outside
 * the n x n view is written.  Non-positive pivot: *host_info = its 1-based index,
 * NaNs propagate like the reference's JAX path; return value 0 unless a HIP error occurred. */
int gpk_potrf(gpk_handle h, double* A, int n, int lda, int* host_info);
int gpk_tril(gpk_handle h, double* A, int n, int lda);
int gpk_symmetrize_lower(gpk_handle h, double* A, int n, int lda);   /* copy lower triangle into the upper */
/* jnp.linalg.solve(self.L, .) with the triangular factor (src/PDEs.py:86,97,143,161,288,306,429,450;
 * src/InverseProblems.py:118-119,145-146): B <- L^{-1} B (trans=0) or L^{-T} B (trans=1); B is n x nrhs. */
int gpk_trsm(gpk_handle h, int trans, const double* L, int n, int ldl, double* B, int nrhs, int ldb);
/* Tall block column A (nrows x ncols, nrows >= ncols <= 512 recommended): the top ncols x ncols block is replaced by its
 * Cholesky factor L (lower) and the rows below by A[ncols:, :] L^{-T} -- one panel step of the blocked factorisation
 * (jnp.linalg.cholesky, src/PDEs.py:77), the owner's share of a step of the panel-sharded multi-GPU factorisation.
 * host_info as gpk_potrf (may be NULL: no host synchronisation then). */
int gpk_potrf_panel(gpk_handle h, double* A, int nrows, int ncols, int lda, int* host_info);
/* The same panel step for schedules that must not touch the host per panel (gpk/sharded.py, look-ahead): the pivot status
 * accumulates in the handle's device-side info word (first failure wins; pivot indices offset by pivot_base = the panel's first
 * column in the whole matrix).  gpk_info_reset before the first panel, ONE gpk_info_read (synchronises) after the last. */
int gpk_potrf_panel_at(gpk_handle h, double* A, int nrows, int ncols, int lda, int pivot_base);
int gpk_info_reset(gpk_handle h);
int gpk_info_read(gpk_handle h, int* host_info);
/* X <- X L^{-T} (X is m x n): the panel solve of the blocked Cholesky; exported for the multi-GPU panel-sharded
 * factorisation, whose per-panel schedule lives in the host layer (gpk/sharded.py). */
int gpk_trsm_right_lt(gpk_handle h, const double* L, int n, int ldl, double* X, int m, int ldx);
/* B <- L^{-T} L^{-1} B (src/PDEs.py:205,347,502; src/InverseProblems.py:190,195) */
int gpk_potrs(gpk_handle h, const double* L, int n, int ldl, double* B, int nrhs, int ldb);
/* C <- alpha*op(A)*op(B) + beta*C; ta/tb = 1 means the operand is stored transposed (op(A) is m x k). */
int gpk_gemm(gpk_handle h, int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda,
             const double* B, int ldb, double beta, double* C, int ldc);
/* Leading-zero variants used by the column-sharded Gauss-Newton step (gpk/sharded.py) on the [A(z) | F] block built by
 * gpk_gn_build_rev: column c < lead of the right-hand side / of operand B is zero above row lead-1-c, columns >= lead are
 * dense.  Same results as gpk_trsm / gpk_gemm(tb = 0); the zeros are skipped (contiguous active column ranges in the
 * solve, late K start per tile in the product).  lead <= 0 degenerates to the dense routines. */
int gpk_trsm_lz(gpk_handle h, const double* L, int n, int ldl, double* B, int nrhs, int ldb, int lead);
int gpk_gemm_lz(gpk_handle h, int ta, int m, int n, int k, double alpha, const double* A, int lda,
                const double* B, int ldb, double beta, double* C, int ldc, int lead);
/* Companion of a Cholesky factor that is reused for many multi-right-hand-side forward solves (the factor of Theta in
 * GN_method: jnp.linalg.solve(self.L, .) inside every Hessian_GN, src/PDEs.py:97,306,450; src/InverseProblems.py:145-146):
 * Dinv (n x block doubles, leading dimension block; block = 256, 512, 1024 or 2048) receives the inverses of the block x block
 * diagonal blocks of L, block k in rows [k block, k block + n_k), computed by substitution.  gpk_trsm_dinv then solves
 * L X = B with GEMMs only: X (n x nrhs, ld ldx, must not alias B) receives L^{-1} B, B is overwritten with intermediate
 * values.  lead > 0: column c < lead of B is zero above row lead-1-c (as gpk_trsm_lz); the zero part of X left of that
 * boundary is NOT written, so X must be zero there on entry (zero X once; solves of the same shape keep it valid).
 * Accuracy: DESIGN.md section 4 (Gauss-Newton iterates within 3e-13 of the substitution path at nugget 1e-13, config 2). */
int gpk_trtri_diag(gpk_handle h, const double* L, int n, int ldl, double* Dinv, int block);
int gpk_trsm_dinv(gpk_handle h, const double* L, const double* Dinv, int block, int n, int ldl, double* B, int nrhs, int ldb,
                  double* X, int ldx, int lead);
/* C <- alpha*A^T A + beta*C, A is k x n row-major; lower triangle only unless full != 0
 * (the 2*ss^T ss of src/PDEs.py:307 and of every autodiff Hessian_GN). */
int gpk_syrk(gpk_handle h, int n, int k, double alpha, const double* A, int lda, double beta, double* C, int ldc, int full);

/* ---- Gauss-Newton ------------------------------------------------------------------------------------------ */
typedef struct {
    int system;              /* GPK_GN_* */
    int Nd, Nb, Ndata;
    double p0, p1;           /* ELLIPTIC(_RELAXED): alpha, m   BURGERS: alpha, nu   EIKONAL: eps, -   DARCY: noise_level, -   SEMILINEAR: eps, -   MONGE_AMPERE: -, -
                              * SEMILINEAR3D: a3, b2 (the coefficients of u g3 and of g2^2)   QUASILINEAR: the first two parameters of its GPK_QL_* kind */
    double pen_lambda;       /* ELLIPTIC_RELAXED: the penalty   SEMILINEAR3D: b3 (the coefficient of g3^2) */
    const double* rhs_f;     /* (Nd,)  */
    const double* bdy_g;     /* (Nb,)  */
    const double* data_u;    /* (Ndata,) DARCY only */
    const double* L;  int ldl;     /* factor of Theta (DARCY: L_u) */
    const double* L2; int ldl2;    /* DARCY: L_a */
    const double* Dinv;            /* optional (may be NULL): gpk_trtri_diag(L)  -- the S solve then runs as GEMMs only */
    const double* Dinv2;           /* optional, DARCY: gpk_trtri_diag(L2) */
    int dinv_block;                /* block size Dinv / Dinv2 were built with (0 = 256) */
    /* optional (may be NULL) -- see gpk_gn_structured_prepare (v0: GPK_GN_ELLIPTIC only) */
    const double* W1; const double* W2; const double* v0; int ldw;
    /* optional (may be NULL), needs W1/W2/v0 -- see gpk_gn_gram_prepare */
    const double* G; int ldg; const double* pvec;
    /* optional (may be NULL), GPK_GN_DARCY only -- see gpk_gn_darcy_prepare */
    const double* Wa; int ldwa; const double* Ha; int ldha;
    /* GPK_GN_SEMILINEAR: the coefficients (a1, a2, b, c1, c3) of N(u, grad u); five consecutive doubles.
     * GPK_GN_SEMILINEAR3D: a1, a2, b1 (in gq_b), c1, c3 -- with a3 = p0, b2 = p1, b3 = pen_lambda the eight coefficients of its N */
    double gq_a1, gq_a2, gq_b, gq_c1, gq_c3;
    /* reaction term of ELLIPTIC(_RELAXED): GPK_NL_* with the parameters p0, p1 above and p2 (CUBIC only); 0 = alpha u^m.
     * QUASILINEAR: the equation kind GPK_QL_* with the parameters p0, p1, p2.  Any other system takes 0 only (-9001 otherwise) */
    int nonlin; double p2;
} gpk_gn_problem;

/* sizes: nz unknowns, rows of the stacked S = [L^{-1}A | L^{-1}F] buffer */
int gpk_gn_dims(const gpk_gn_problem* host_prob, int* nz, int* s_rows);
/* Workspace query (pure host function, no device): what a caller has to allocate for gpk_gn_step / gpk_gn_hessian_grad and what the
 * handle will reserve by itself.  lds: the leading dimension the caller intends to use for S and Hb (0 = the smallest admissible one,
 * nz + 1 rounded up to 16 doubles; returned in *host_lds).  *S_bytes = s_rows * lds * 8, *Hb_bytes = (nz + 1) * lds * 8, *delta_bytes =
 * nz * 8, *handle_bytes = the out-of-place solve buffer the handle grows on first use when the inverted diagonal blocks of EVERY factor are
 * supplied (s_rows * lds * 8 -- whatever dinv_block says, 0 meaning 256 -- else 0; + s_rows * 8 for the exact in-step loss).  An UPPER
 * BOUND on the large buffers (the loss vector is counted whether or not gpk_tune key 52 is on); on top of it the handle keeps two sets
 * of hand-off records of its single-vector solves (2 x 4 MB, fixed) once the in-step loss runs on its side stream.  Any output pointer may be NULL. */
int gpk_gn_worksize(const gpk_gn_problem* host_prob, int lds, int* host_lds, size_t* S_bytes, size_t* Hb_bytes, size_t* delta_bytes,
                    size_t* handle_bytes);
/* (With host_prob->Dinv set, S is scratch and the solved block lives in the handle's workspace.) */
/* One Gauss-Newton step = Hessian_GN + grad_loss + linear solve + update (src/PDEs.py:117-119,322-325,472-475;
 * src/InverseProblems.py:164-166) and the loss of the INPUT iterate (src/PDEs.py:82-87 ...):
 *   S  = [L^{-1}A(z) | L^{-1}F(z)]                (s_rows x (nz+1), ld lds)
 *   Hb = S^T S  (bordered: H/2, g/2, loss)        ((nz+1) x (nz+1), ld ldh)
 *   z <- z - step * H^{-1} g                       via Cholesky of Hb
 * host_loss_in = loss(z_in) = sum_k ||L_k^{-1} F_k(z_in)||^2 by TRUE SUBSTITUTION with the factor(s) (one vector; exact to rounding like
 * gpk_gn_loss -- rounds 2-4 returned the squared norm of the F column of the GEMM-only solve instead, ~1e-8 relative error at nugget
 * <= 1e-12 near convergence; since round 6 the structured modes below report the substituted value as well).  WHERE it runs: F(z_in) is
 * written at the start of the call on the handle's stream; from the second call of a handle on, the substitution chain (one single-vector
 * solve per factor + a dot product) is issued on an INTERNAL side stream of the handle (the CU-masked stream of the pipelined phase),
 * next to the end of the step, and joined before the call returns -- the call is still synchronous for the caller and ordered on the
 * handle's stream, but a profiler shows a second stream; the first call of a handle, handles without the two-partition pipeline and
 * gpk_tune(h, 52, 2) run the chain on the handle's stream in front of the solve phase.  host_info = potrf info of H (0 ok).
 * delta (nz,) receives H^{-1} g.  One call = one iteration of the
 * reference's GN_method loop (Hessian, gradient, solve, update, one loss evaluation). */
int gpk_gn_step(gpk_handle h, const gpk_gn_problem* host_prob, double* z, double step_size,
                double* S, int lds, double* Hb, int ldh, double* delta, double* host_loss_in, int* host_info);
/* ---- Backtracking line search for the Gauss-Newton iteration ("Line search").  No reference call site: the
 *      reference's loop takes a fixed step size.  With delta = H^{-1} g and y = L_H^{-1} g / 2 (the last row of the factored Hb),
 *        J(z - t delta) ~ J(z) - 2 t |y|^2 + t^2 |y|^2     (the Gauss-Newton model along delta; g . delta = 2 |y|^2),
 *      and a trial loss J(z - t_k delta) is a measurement vector pushed through the fixed factor(s) of Theta: K trials are ONE K-column
 *      forward solve.  All entries refuse bad arguments with -9001 (named in gpk_last_error) before anything is launched, serve every
 *      system gpk_gn_loss serves and take the GEMM-only solve when the problem carries Dinv / Dinv2. */
#define GPK_LS_MAX_TRIALS 16
typedef struct { int K; double t0, beta, c1; } gpk_ls_options;   /* zeros mean the defaults 8, 1.0, 0.5, 1e-4 */
/* gpk_gn_step with the update left out: the same mode selection, the same launches, the same side-stream loss chain.  z is not written;
 * delta, *host_loss_in and *host_info are what gpk_gn_step returns (bit for bit), *host_pred = |y|^2 = g . delta / 2 (a device dot product
 * over the last row of the factored Hb): J - pred is the minimum of the linearised loss.  One host synchronisation. */
int gpk_gn_direction(gpk_handle h, const gpk_gn_problem* host_prob, const double* z, double* S, int lds, double* Hb, int ldh,
                     double* delta, double* host_loss_in, double* host_pred, int* host_info);
/* Workspace query (pure host function) for K trials: ldw = the leading dimension the caller intends to use for W (0 = K rounded up to
 * 16 doubles; returned in *host_ldw); *bytes = what W must hold: the K right-hand sides (s_rows x ldw), the out-of-place result of the
 * GEMM-only solve (the same again, when every factor comes with its inverted diagonal blocks) and the partial sums of the reduction. */
int gpk_gn_trial_worksize(const gpk_gn_problem* host_prob, int K, int ldw, int* host_ldw, size_t* bytes);
/* dev_losses[k] = J(z - host_t[k] delta), k < K, 1 <= K <= GPK_LS_MAX_TRIALS: one launch writes the K measurement vectors F(z - t_k delta)
 * as the columns of W (the step sizes travel in the kernel arguments; the trial point is formed by the expression the update uses, so an
 * accepted iterate is bit for bit the point that was measured), one K-column forward solve per factor, column sums of squares.  Of W only
 * the first K columns of its rows are written, of dev_losses only K doubles.  host_losses may be NULL: then nothing is downloaded and the
 * call does not synchronise. */
int gpk_gn_trial_losses(gpk_handle h, const gpk_gn_problem* host_prob, const double* z, const double* delta, const double* host_t, int K,
                        double* W, int ldw, double* dev_losses, double* host_losses);
/* Acceptance on the device: trials in the order given; the first k whose loss is finite and <= loss_in - 2 c1 t_k pred; if there is none,
 * the k of the smallest finite loss provided that loss is < loss_in; otherwise k = -1.  Then z <- z - t_k delta (k = -1: z is not
 * touched).  *host_k, *host_t_acc (0 for k = -1) come back with one download. */
int gpk_gn_trial_accept(gpk_handle h, int nz, double* z, const double* delta, const double* dev_losses, const double* host_t, int K,
                        double loss_in, double pred, double c1, int* host_k, double* host_t_acc);
/* One line-searched step = gpk_gn_direction + gpk_gn_trial_losses + gpk_gn_trial_accept with t_k = t0 beta^k (t_{k+1} = t_k * beta, one
 * rounding per trial), all on the device with ONE host synchronisation; the Armijo test uses the substituted loss of the input iterate
 * (the side-stream chain is joined in front of the acceptance).  opt may be NULL (all defaults).  host_losses: K doubles (may be NULL).
 * *host_info != 0 (the factorisation of H failed) gives *host_k = -1 and no update. */
int gpk_gn_step_ls(gpk_handle h, const gpk_gn_problem* host_prob, double* z, const gpk_ls_options* opt, double* S, int lds, double* Hb, int ldh,
                   double* delta, double* W, int ldw, double* host_loss_in, double* host_losses, int* host_k, double* host_t_acc,
                   int* host_info);
/* OPTIONAL structured solve of the elliptic system (not what the reference does per step; off unless W1/W2/v0 are set).  A(z) =
 * [diag(alpha m z^(m-1)); I; 0] has its non-zeros in fixed places and the solve is linear in the right-hand sides, so with
 *   W1 = L^{-1} [I; 0; 0],  W2 = L^{-1} [0; I; 0]   (s_rows x nz each, leading dimension ldw >= nz+1, columns in the internal order of
 *   gpk_gn_step),  v0 = L^{-1} F(0)  (s_rows)
 * computed ONCE by this call (two solves; S is scratch, s_rows x lds), every later gpk_gn_step whose host_prob carries W1, W2, v0, ldw
 * forms  S = [W1 diag(tau'(z)) + W2 | v0 + W1 (tau(z) - tau(0)) + W2 z]  in one memory-bound pass instead of the triangular solve
 * (F(0) carries tau(0), which is p0 for GPK_NL_EXP and 0 for every other kind).  Same
 * iterates up to rounding (tests/test_gpu_structured.py); the product, the factorisation and the update are unchanged.
 * Systems other than the elliptic one (round 6: GPK_GN_BURGERS, GPK_GN_EIKONAL, GPK_GN_DARCY; needs Dinv / Dinv2 / dinv_block, i.e. the
 * GEMM-only solve path and its leading-zero layout).  Every column of their A(z) has at most ONE entry that depends on z -- Burgers:
 * the PDE row (-alpha v2, -alpha v0, nu: src/PDEs.py:297-299 of the reference), Eikonal: 2 v1 / eps, 2 v2 / eps (:443-445), Darcy: the
 * v3 row of the u-part (f e^{-w0}, -v1, -v2, -w1, -w2: src/InverseProblems.py:131-135) -- so A(z) = A1 diag(d(z)) + A2 with constant
 * 0/1 patterns, and  W1 = L^{-1} A1,  W2 = L^{-1} A2  (all row groups stacked, s_rows x (nz+1) each, ldw even and >= nz+1; v0 is not
 * used and may be NULL) are computed ONCE here.  Every later gpk_gn_step whose host_prob carries W1, W2, ldw forms
 * L^{-1}A(z) = W1 diag(d(z)) + W2 in one memory-bound pass; the column L^{-1}F(z) is still SOLVED every step (one column per factor).
 * Same iterates up to rounding (tests/test_gpu_structured.py: <= 1e-8 relative to the per-step solve, <= 1e-6 to the oracle). */
int gpk_gn_structured_prepare(gpk_handle h, const gpk_gn_problem* host_prob, double* S, int lds, double* W1, double* W2, double* v0, int ldw);
/* OPTIONAL second level of the structured mode (elliptic system): with the Gram blocks of W = [W1 W2],
 *   G = [G11; G12; G21; G22]  (four nz x nz blocks stacked, leading dimension ldg >= nz; Gij = Wi^T Wj),
 *   pvec = [W1^T v0 (nz); W2^T v0 (nz); v0^T v0 (1)],
 * computed ONCE by this call from W1, W2, v0 (host_prob must carry them), gpk_gn_step assembles the bordered matrix directly,
 *   H/2 = D G11 D + D G12 + G21 D + G22,   g/2 = D q1 + q2,   loss = v0^T v0 + a.p1 + z.p2 + a.q1 + z.q2
 *   (D = diag(tau'(z)), a = tau(z) - tau(0) -- alpha m z^(m-1) and alpha z^m for the power law --, q1 = G11 a + G12 z + p1, q2 = G21 a + G22 z + p2),
 * in O(nz^2) memory-bound work per step: neither the triangular solve nor the product S^T S is executed; the Cholesky
 * factorisation of H, the solve and the update are unchanged.  Same iterates up to rounding (tests/test_gpu_structured.py).
 * Burgers / Eikonal / Darcy (round 6; host_prob carries the W1, W2 of their structured form, A(z) = A1 diag(d(z)) + A2): the same four
 * blocks; per step  H/2 = D G11 D + D G12 + G21 D + G22  with D = diag(d(z)), and the border from the column w = L^{-1}F(z), which is
 * SOLVED every step (one column per factor):  g/2 = D W1^T w + W2^T w,  loss = w^T w.  pvec (2 nz + 1) is zeroed and not used.
 * H of these systems is ill-conditioned (1e10 .. 1e12) -- the assembled form agrees with S^T S to 1e-14 relative and the steps to
 * 1e-10 (tests/test_gpu_structured.py), inside the 1e-6 parity bound, but it is opt-in like every structured mode. */
int gpk_gn_gram_prepare(gpk_handle h, const gpk_gn_problem* host_prob, double* G, int ldg, double* pvec);
/* Darcy system: the iteration-independent part of the step, computed ONCE per factor (round 6).  The a-part rows of GN_loss,
 * [w1; w2; w0] against L_a (src/InverseProblems.py:137-146 of the reference), do not involve z_old: their block of A(z) is a
 * permutation matrix, so W_a = L_a^{-1} A_a and its contribution H_a = W_a^T W_a to the Gauss-Newton matrix are the same in every
 * step -- the reference recomputes them inside every Hessian_GN because autodiff cannot know.  This call runs exactly the launches a
 * step would (same kernels, same shapes) and keeps their results:
 *   Wa (3 N_d x 3 N_d, ld ldwa >= 3 N_d): the solved a-part block in the step's internal column order; must not alias S;
 *   Ha (3 N_d x 3 N_d, ld ldha >= 3 N_d): the lower triangle of W_a^T W_a;
 * S (s_rows x lds) is scratch.  A gpk_gn_step whose host_prob carries Wa/ldwa/Ha/ldha then skips the a-part's 3 N_d-column solve and
 * its product (an O(N_d^2) add instead); the a-part's F column (which depends on z) is still solved every step.  The iterates are
 * BIT-IDENTICAL to the uncached step (tests/test_gpu_structured.py).  Needs Dinv / Dinv2 (the GEMM-only solve path); on the other
 * paths the fields are ignored.  The caller must drop Wa / Ha when L2 is refactored. */
int gpk_gn_darcy_prepare(gpk_handle h, const gpk_gn_problem* host_prob, double* S, int lds, double* Wa, int ldwa, double* Ha, int ldha);
/* building blocks of gpk_gn_step for the column-sharded multi-GPU step: S <- [A(z) | F(z)] (no solve), y += alpha x */
int gpk_gn_build(gpk_handle h, const gpk_gn_problem* host_prob, const double* z, double* S, int lds);
/* Same with unknown j stored in column n_z-1-j (elliptic system): column c < n_z of [A | F] is then zero above row
 * n_z-1-c -- the layout gpk_gn_step uses internally and gpk_trsm_lz / gpk_gemm_lz exploit.  Round 6: also the Eikonal, Burgers and
 * Darcy systems, in the staircase orders of THEIR gpk_gn_step (unknown groups v1, v2, v0 / the three unknowns of a point interleaved /
 * v1, v2, w1, w2, w0, v0). */
int gpk_gn_build_rev(gpk_handle h, const gpk_gn_problem* p, const double* z, double* S, int lds);
int gpk_axpy(gpk_handle h, int n, double alpha, const double* x, double* y);
/* loss(z) (src/PDEs.py:82-87,278-289,418-430,138-147; src/InverseProblems.py:105-120); work: s_rows doubles. */
int gpk_gn_loss(gpk_handle h, const gpk_gn_problem* host_prob, const double* z, double* work, double* host_loss);
/* Hessian_GN(z,z) and grad_loss(z) as the reference returns them (full symmetric H = 2 A^T Theta^{-1} A, g);
 * H is nz x nz with ld ldh (needs (nz+1) x ldh storage, ldh >= nz+1), g (nz,). */
int gpk_gn_hessian_grad(gpk_handle h, const gpk_gn_problem* host_prob, const double* z,
                        double* S, int lds, double* H, int ldh, double* g);
/* measurement vector(s) F(z) = sol_vec (src/PDEs.py:132-134,338-342,488-497; IP.py:176-186): out (s_rows,) */
int gpk_gn_measurement(gpk_handle h, const gpk_gn_problem* host_prob, const double* z, double* out);

/* ---- Posterior variance of the GP solution at test points, Gauss-Newton / Laplace form ("Posterior variance").
 *      No reference call site: the reference returns the posterior mean only.  With A = dF/dz at the final iterate z*, L L^T = Theta and
 *      H/2 = A^T Theta^{-1} A (what gpk_gn_hessian_grad returns, halved; Darcy's data term included),
 *        var(x) = 1 - ||L^{-1} k_x||^2 + ||L_H^{-1} A^T Theta^{-1} k_x||^2,   L_H L_H^T = H/2,
 *                 `--- var_cond ----'   `---------- var_gn ----------'
 *      k_x = the covariances of u(x) with the N collocation functionals (k(x,x) = 1 for both kernels).  The value functional only; the
 *      five reference layouts; GPK_GN_ELLIPTIC_RELAXED is not served (-9001).  Bad arguments: -9001, named in gpk_last_error. */
/* The block of gpk_assemble_test transposed: out is N x Nt row-major, ld >= Nt, out[c * ld + t] = Theta_test[t, c] -- the layout
 * gpk_trsm / gpk_trsm_dinv take as B, so no transpose pass exists anywhere.  Any alignment of out / ld is accepted (16-byte stores
 * when base, ld and Nt allow; 8-byte stores otherwise, with the same values); nothing outside the N x Nt view is written.  The launch is
 * not part of the per-phase timing: gpk_prof_read_assembly keeps reporting the last Gram launch. */
int gpk_assemble_cross(gpk_handle h, int layout, int kernel, const double* host_kparams,
                       const double* Xt, int Nt, const double* Xd, int Nd, const double* Xb, int Nb,
                       double* out, int ld);
/* out[t] = (base ? base[t] : 0) + alpha * sum_r V[r, t]^2 for the rows x cols view V (ld ldv >= cols); base may be out.  One pass over
 * V; the rows are cut into a number of slabs that depends on (rows, cols) only and the partial sums are added in slab order: no
 * atomics, a repeated call gives bit-identical output.  Uses the handle's workspace for the partial sums. */
int gpk_col_sumsq(gpk_handle h, const double* V, int rows, int cols, int ldv, double alpha, const double* base, double* out);
/* Workspace query (pure host function) for the two calls below with batches of nt test points.  ldp / ldr / ldk: the leading dimensions
 * the caller intends to use for P / R / K and W (0 = the smallest admissible one -- nz + 1, nz, nt -- rounded up to 16 doubles; returned
 * in *host_ld*).  *P_bytes = s_rows * ldp * 8, *R_bytes = nz * ldr * 8, *K_bytes = (rows of the largest field) * ldk * 8, *W_bytes =
 * nz * ldk * 8, *handle_bytes = what the two calls ask of the handle's workspace, computed by the functions they size it with: the
 * larger of prepare's [A | F] block (s_rows * ldp * 8, when every factor comes with its inverted diagonal blocks) and variance's
 * out-of-place V (N_field * ldk * 8, when the field's factor has them) plus the partial sums of the reductions; 0 inverted blocks: the
 * partial sums alone.  Any output pointer may be NULL. */
int gpk_posterior_worksize(const gpk_gn_problem* host_prob, int nt, int ldp, int ldr, int ldk, int* host_ldp, int* host_ldr,
                           int* host_ldk, size_t* P_bytes, size_t* R_bytes, size_t* K_bytes, size_t* W_bytes, size_t* handle_bytes);
/* Once per converged iterate z:  P <- L^{-1} A(z) (s_rows x nz in the natural column order of gpk_gn_build, every row group solved with
 * its own factor, the rows without a factor copied; ld ldp >= nz + 1 -- column nz is scratch),  R <- the lower Cholesky factor of
 * H/2 (nz x nz, ld ldr >= nz; strict upper triangle unspecified, as gpk_potrf).  H/2 is formed as P^T P with Darcy's data rows
 * (1 / gamma, no factor) kept in P: the product gpk_gn_hessian_grad issues, without its border column and its factor 2.  The solve
 * takes gpk_gn_hessian_grad's path: GEMMs only when every factor comes with its inverted diagonal blocks, substitution otherwise.
 * host_info as gpk_potrf. */
int gpk_posterior_prepare(gpk_handle h, const gpk_gn_problem* host_prob, const double* z, double* P, int ldp, double* R, int ldr,
                          int* host_info);
/* One batch of nt test points.  field: 0 = u, 1 = a (GPK_GN_DARCY only: factor L2, the a-rows of P; anything else -9001).  K: N_field x
 * nt from gpk_assemble_cross (ld ldk >= nt), OVERWRITTEN;  W: nz x nt scratch (ld ldw >= nt).
 *   V = L_field^{-1} K;  var_cond[t] = 1 - sum_r V[r,t]^2;  W = P_field^T V;  W <- R^{-1} W;  var[t] = var_cond[t] + sum_r W[r,t]^2.
 * var_cond, var: (nt,) on the device, either may be NULL (var == NULL: steps 3-5 are skipped and P, R, W are not read).  Raw values,
 * nothing is clipped. */
int gpk_posterior_variance(gpk_handle h, const gpk_gn_problem* host_prob, const double* P, int ldp, const double* R, int ldr, int field,
                           double* K, int ldk, int nt, double* W, int ldw, double* var_cond, double* var);

/* ---- Posterior covariance between test points and samples of the posterior ("Posterior covariance and samples").
 *      No reference call site.  With k_s, k_t the columns of gpk_assemble_cross for the test points x_s, x_t,
 *        Sigma[s,t] = k(x_s, x_t) - (L^{-1} k_s)^T (L^{-1} k_t) + (L_H^{-1} A^T Theta^{-1} k_s)^T (L_H^{-1} A^T Theta^{-1} k_t),
 *      whose diagonal is var of the section above.  The value functional, the five kernels of the reference layouts, one batch of test
 *      points (no blocks between two batches); GPK_GN_ELLIPTIC_RELAXED is not served (-9001).  Bad arguments: -9001, named in gpk_last_error. */
/* out[i * ld + j] = k(xa_i, xb_j) for the na points Xa and the nb points Xb ((n, 2) row-major, on the device; Xa == Xb allowed), ld >= nb.
 * host_kparams as for gpk_assemble.  Every entry is computed from its own xa_i - xb_j (nothing is mirrored); k is even in it, so with
 * Xa == Xb out[i][j] and out[j][i] are the same bits and the diagonal is exactly 1.  Any alignment of out / ld is accepted (16-byte
 * stores when base, ld and nb allow and gpk_tune key 47 is on; 8-byte stores otherwise, with the same bits); nothing outside the na x nb
 * view is written.  Write-bound: 8 na nb bytes. */
int gpk_assemble_prior(gpk_handle h, int kernel, const double* host_kparams, const double* Xa, int na, const double* Xb, int nb,
                       double* out, int ld);
/* One batch of nt test points.  On entry C (nt x nt, ld ldc >= nt) holds the prior gpk_assemble_prior(Xt, Xt) and K (N_field x nt, ld
 * ldk >= nt) the block of gpk_assemble_cross, OVERWRITTEN; W: nz x nt scratch (ld ldw >= nt).  On return
 *   C = C - V^T V + W^T W,   V = L_field^{-1} K,   W = R^{-1} P_field^T V,
 * V and W formed by the calls of gpk_posterior_variance (same solve path, same workspace: gpk_posterior_worksize with this nt), the two
 * products by the routine under gpk_syrk (alpha = -1 / +1, beta = 1, lower triangle), then gpk_symmetrize_lower: both triangles are
 * written and C[s][t], C[t][s] are the same bits.  with_gn == 0: the conditional covariance C - V^T V alone; P, R and W are not read
 * and may be NULL.  field as gpk_posterior_variance.  Raw values, nothing is clipped. */
int gpk_posterior_covariance(gpk_handle h, const gpk_gn_problem* host_prob, const double* P, int ldp, const double* R, int ldr, int field,
                             double* K, int ldk, int nt, double* W, int ldw, double* C, int ldc, int with_gn);
/* ns samples of N(mean, C + jitter I) at nt points:  C <- C + jitter I,  C <- its lower Cholesky factor (gpk_potrf, gpk_tril),
 * out[t * ldo + s] = mean[t] + (L Xi)[t, s]  (out nt x ns, ld ldo >= ns; the product is gpk_gemm with beta = 1 on the broadcast mean).
 * Xi (nt x ns, ld ldxi >= ns): standard normals SUPPLIED BY THE CALLER -- the library draws nothing, so a sample is a pure function of
 * its inputs and repeats to the bit.  jitter >= 0 is absolute, in units of the prior variance k(x,x) = 1.  *host_info as gpk_potrf
 * (may be NULL); the call reads the pivot status back before it writes (it synchronises once): with info != 0 out is left unwritten
 * and the call returns 0.  C is overwritten either way. */
int gpk_posterior_sample(gpk_handle h, double* C, int ldc, int nt, double jitter, const double* mean, const double* Xi, int ldxi, int ns,
                         double* out, int ldo, int* host_info);

/* ---- Log evidence of a factored problem at its Gauss-Newton iterate, Laplace form ("Log evidence").
 *      No reference call site: the reference takes the kernel parameter by hand.  With F(z) the stacked measurement vector (s_rows),
 *      A = dF/dz at the final iterate z*, L_k L_k^T = Theta_k for each factor (one; L_a and L_u for GPK_GN_DARCY),
 *      J(z) = sum_k ||L_k^{-1} F_k(z)||^2 (+ Darcy: ||v0[:N_data] - data||^2 / gamma^2, what gpk_gn_loss returns) and
 *      H/2 = A^T Theta^{-1} A = R R^T (what gpk_posterior_prepare forms, Darcy's data rows kept in), the Laplace approximation of
 *      the integral of N(F(z); 0, Theta) over z around z* is
 *        log Z = -J(z*)/2 - sum_k sum_i log (L_k)_ii - sum_i log R_ii - N_data log gamma - (s_rows - nz)/2 log 2 pi,
 *      s_rows - nz = N_d + N_b (+ N_data) being the number of data values f, g (and observations).  When F is affine in z this is exact:
 *      |Theta| |A^T Theta^{-1} A| = |Theta_dd| makes it the Gaussian log likelihood of the data rows d under their own block Theta_dd,
 *      whatever z.  Bad arguments: -9001, named in gpk_last_error. */
/* *host_logdet = 2 sum_i log L_ii = log |L L^T| of the n x n lower factor L (ld ldl >= n, any alignment); only the diagonal is read
 * (stride ldl + 1).  *host_bad = the number of diagonal entries that are not > 0 (NaN included); the sum is then what IEEE arithmetic
 * gives (log 0 = -inf, log of a negative number = NaN).  Fixed reduction order -- strided partial sums per lane, wave shuffles, LDS
 * across the waves of a workgroup, the workgroups' partial sums added in index order -- and no atomics: a repeated call and a fresh handle
 * give the same bits.  Synchronises, as gpk_gn_loss.  Uses the handle's workspace for the partial sums. */
int gpk_chol_logdet(gpk_handle h, const double* L, int n, int ldl, double* host_logdet, int* host_bad);
/* gpk_gn_loss (work: s_rows doubles), gpk_posterior_prepare into the caller's P / R (sizes and leading dimensions:
 * gpk_posterior_worksize) and gpk_chol_logdet's reduction over every factor and over R.
 *   host_terms[6] = { log Z,  J(z),  sum_k log |Theta_k|,  log |H/2|,  N_data log gamma,  (s_rows - nz)/2 log 2 pi },
 *   log Z = -(terms[1] + terms[2] + terms[3]) / 2 - terms[4] - terms[5].
 * *host_info is prepare's; if it is non-zero, or a diagonal entry of a factor or of R is not > 0, log Z is NaN -- the call still returns 0
 * and the other five terms are what the arithmetic gave.  P and R are left exactly as gpk_posterior_prepare leaves them (a following
 * gpk_posterior_variance may use them).  GPK_GN_ELLIPTIC_RELAXED is not served (-9001, prepare's message). */
int gpk_log_evidence(gpk_handle h, const gpk_gn_problem* host_prob, const double* z, double* P, int ldp, double* R, int ldr,
                     double* work, double* host_terms, int* host_info);

/* Development switches, phase stamps, probes and the micro-benchmarks behind the roofline denominators: include/gpk_debug.h. */

#ifdef __cplusplus
}
#endif
#endif /* GPK_H */
