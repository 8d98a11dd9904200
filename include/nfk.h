/*
 * nfk.h -- C ABI of libnfk.so, the MI355X (gfx950) kernels of the
 * normalizing-flow coupling-layer hot path.
 *
 * The reference (sherryli59/NormalizingFlow) is pure PyTorch and has no FFI:
 * each entry point below replaces a chain of ATen ops behind one of its Python
 * functions (file:line cited per function).  The Python host layer
 * (normalizingflow_amd/, re-exported as nf/) binds these with ctypes; see
 * INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is device memory owned by the caller (the library never
 *     allocates or frees); fp32 unless the type says otherwise;
 *   - "ld*" arguments are row strides in ELEMENTS;
 *   - logdet_mode: 0 = do not touch logdet, 1 = logdet[b] = v, 2 = logdet[b] += v;
 *   - work is enqueued on `stream` (a hipStream_t); no call synchronises;
 *   - return value: 0 on success, a hipError_t (>0) from the launch, or
 *     NFK_EINVAL (<0) for bad arguments (nfk_last_error() says which).
 *   - data-dependent errors of the reference are recorded, not raised, as bits
 *     in *status (nullable) so the hot path never syncs; the host checks them
 *     lazily (see NFK_ST_*).
 */
#ifndef NFK_H_
#define NFK_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nfk_stream_t; /* hipStream_t */

#define NFK_ABI_VERSION 4
#define NFK_EINVAL (-1)

/* status bits, OR-ed into *status by the kernels */
#define NFK_ST_INSIDE_SEEN 1 /* >=1 element inside [-B, B]; absent => the reference's
                                RuntimeError from torch.min of an empty tensor (utils.py:63) */
#define NFK_ST_NEG_DISC 2    /* negative discriminant in an inverse spline: the
                                reference's AssertionError (utils.py:121) */
#define NFK_ST_NAN_Z 4       /* a NaN in z reached the Normal prior: the reference's
                                ValueError from torch's MultivariateNormal argument
                                validation (prior.log_prob, nf/models.py:19) */

int nfk_abi_version(void);
const char* nfk_last_error(void);

/* ---------------------------------------------------------------------------
 * Rational-quadratic spline coupling.
 * Replaces NSF_CL.forward / NSF_CL.inverse minus the conditioner
 * (nf/flows.py:227-239, 241-253), unconstrained_RQS (nf/utils.py:27-56),
 * RQS (nf/utils.py:58-152) and searchsorted (nf/utils.py:20-25).
 *
 *   params     dense [batch, n_up, 3K-1]: per transformed element the
 *              (W[K], H[K], D[K-1]) block, i.e. psi(lower) reshaped as at
 *              flows.py:231, or cat(W, H, D) for the bare unconstrained_RQS.
 *   param_mode 0: raw NSF_CL conditioner output: W,H <- (right-left)*softmax,
 *                 D <- softplus (flows.py:233-235, where right-left = 2B)
 *                 before the spline's own normalisation;
 *              1: already the unconstrained_RQS arguments (utils.py:27);
 *              2: the bare RQS arguments (utils.py:58): params [batch, n_up, 3K+1]
 *                 with all K+1 derivative logits (no boundary constant).
 *   bounds     knots span [left, right] x [bottom, top] (utils.py:58-60)
 *   tails      1: identity outside [left, right] (unconstrained_RQS, which
 *                 passes left=bottom=-B, right=top=B); 0: every element is
 *                 splined (RQS; the caller checks the domain like utils.py:63)
 *   up_in[j]   column of x holding transformed element j; up_out[j] its column in z
 *   lo_in/lo_out: identity-copied ("lower") columns; n_lo may be 0.
 *   x and z must not alias.
 *   lad_out    nullable per-element log|det| [batch, n_up] with row stride ld_lad
 *   logdet     per-sample sum over j of log|det| (flows.py:238), per logdet_mode
 * ------------------------------------------------------------------------- */
int nfk_rqs_coupling(const float* x, int64_t ldx, const float* params,
                     const int32_t* up_in, const int32_t* up_out, int32_t n_up,
                     const int32_t* lo_in, const int32_t* lo_out, int32_t n_lo,
                     float* z, int64_t ldz, float* logdet, int32_t logdet_mode,
                     float* lad_out, int64_t ld_lad, int64_t batch, int32_t K,
                     double left, double right, double bottom, double top, int32_t tails,
                     double min_bin_width, double min_bin_height, double min_derivative,
                     int32_t param_mode, int32_t inverse, int32_t* status,
                     nfk_stream_t stream);

/* Backward (vector-Jacobian product) of nfk_rqs_coupling: same x / params /
 * maps / spline arguments as the forward call, plus the upstream gradients
 *   gz [batch, ldgz]   dL/dz (may be NULL: 0),  glogdet [batch] dL/dlog|det|
 *   (may be NULL: 0).
 * Writes gparams (dense, the layout of params) = dL/dparams, and
 *   gx[:, up_in[j]] = dL/dx_up,  gx[:, lo_in[q]] = gz[:, lo_out[q]]
 * (the conditioner's contribution to the lower coordinates is added by the
 * caller after its own backward).  No status words: the forward reported them.
 * Replaces the autograd graph of nf/flows.py:227-253 + nf/utils.py:27-152. */
int nfk_rqs_coupling_bwd(const float* x, int64_t ldx, const float* params,
                         const int32_t* up_in, const int32_t* up_out, int32_t n_up,
                         const int32_t* lo_in, const int32_t* lo_out, int32_t n_lo,
                         const float* gz, int64_t ldgz, const float* glogdet,
                         float* gparams, float* gx, int64_t ldgx, int64_t batch, int32_t K,
                         double left, double right, double bottom, double top, int32_t tails,
                         double min_bin_width, double min_bin_height, double min_derivative,
                         int32_t param_mode, int32_t inverse, nfk_stream_t stream);

/* MAF (nf/flows_1.py:159-195): per-coordinate affine map of the columns
 * [c0, c1) with (mu_i, alpha_i) = init_param[0..1] for i = 0 and
 * params[b*ldp + 2*(i - max(c0,1)) + {0,1}] (the conditioner outputs) otherwise.
 *   forward: out[b, dim-1-i] = (x[b,i] - mu_i) / exp(alpha_i),  log|det| -= alpha_i
 *   inverse: out[b, i] = mu_i + exp(alpha_i) * x[b, dim-1-i],   log|det| += alpha_i
 * (the output flip of flows_1.py:183 and the input flip of :187 are folded in).
 * The inverse is sequential in i: call it once per column after the
 * conditioner of that column has read out[:, :i]. */
int nfk_maf(const float* x, int64_t ldx, const float* init_param, const float* params,
            int64_t ldp, int32_t c0, int32_t c1, int32_t dim, float* out, int64_t ldo,
            float* logdet, int32_t logdet_mode, int64_t batch, int32_t inverse,
            nfk_stream_t stream);

/* ActNorm (nf/flows_1.py:198-215): z = x*exp(log_sigma) + mu (inverse
 * (z - mu)/exp(log_sigma)); log|det| = +-sum(log_sigma), a scalar, written to
 * ld_scalar (may be NULL) and/or written/accumulated into logdet[batch]. */
int nfk_actnorm(const float* x, int64_t ldx, const float* mu, const float* log_sigma,
                int32_t dim, float* z, int64_t ldz, float* logdet, int32_t logdet_mode,
                float* ld_scalar, int64_t batch, int32_t inverse, nfk_stream_t stream);

/* searchsorted (nf/utils.py:20-25), including its side effect:
 *   bin_locations[r, n_loc-1] += eps  (in place, fp32), then
 *   idx[r] = #{j : inputs[r] >= bin_locations[r, j]} - 1
 * bin_locations: dense [rows, n_loc]; inputs, idx: [rows]. */
int nfk_searchsorted(float* bin_locations, const float* inputs, int64_t* idx, int64_t rows,
                     int32_t n_loc, double eps, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Affine half-coupling of RealNVP (nf/flows.py:52-76):
 *   forward: out = t + in * exp(s),       logdet (+)= sum_j s
 *   inverse: out = (in - t) * exp(-s),    logdet (+)= sum_j (-s)
 * in/out may alias.  s and t share the row stride ld_st.
 * ------------------------------------------------------------------------- */
int nfk_affine_coupling(const float* x_in, int64_t ld_in, const float* s, const float* t,
                        int64_t ld_st, float* x_out, int64_t ld_out, float* logdet,
                        int32_t logdet_mode, int64_t batch, int32_t n, int32_t inverse,
                        nfk_stream_t stream);

/* Backward of nfk_affine_coupling (the VJP of flows.py:56/61 and 68/74 for
 * RealNVP's training path):
 *   forward  out = t + in e, e = exp(s):    g_in (+)= g e, g_t = g,    g_s = g in e + g_ld
 *   inverse  out = (in - t) e, e = exp(-s): g_in (+)= g e, g_t = -g e, g_s = -g out - g_ld
 * g = g_out (NULL: 0), g_ld = g_logdet[row] (NULL: 0); g_in written
 * (accumulate = 0) or added to (1); g_t may be NULL forward (it equals g_out).
 * g_s and g_t share the row stride ld_gst. */
int nfk_affine_coupling_bwd(const float* x_in, int64_t ld_in, const float* s, const float* t,
                            int64_t ld_st, const float* g_out, int64_t ld_g, const float* g_logdet,
                            float* g_in, int64_t ld_gin, int32_t accumulate, float* g_s, float* g_t,
                            int64_t ld_gst, int64_t batch, int32_t n, int32_t inverse,
                            nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Planar flow forward (nf/flows_1.py:42-60), parameters w,u [dim], b [1].
 * nonlinearity: 0 tanh (u re-parameterised to u_hat), 1 leaky_relu, 2 elu
 * (u used as is; derivative exactly as flows_1.py:12-18, incl. its -0.01).
 * log|det| = log(|1 + phi.u_hat| + 1e-4).
 * ------------------------------------------------------------------------- */
int nfk_planar(const float* x, int64_t ldx, const float* w, const float* u, const float* b,
               float* z, int64_t ldz, float* logdet, int32_t logdet_mode, float* ld_out,
               int64_t batch, int32_t dim, int32_t nonlinearity, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Radial flow (nf/flows_1.py:85-97).  Its r = ||x - x0||_F is a BATCH-GLOBAL
 * norm, so the flow is two calls with an optional cross-rank all-reduce of
 * *sumsq in between:
 *   nfk_radial_sumsq: *sumsq = sum_{b,i} (x[b,i]-x0[i])^2 (fp64, deterministic;
 *                     workspace >= nfk_radial_workspace_elems() doubles)
 *   nfk_radial_apply: z = x + beta_hat*h*(x-x0); ld_scalar[0] = log|det|
 *                     (identical for every sample, shape [1] as in the reference)
 * ------------------------------------------------------------------------- */
int64_t nfk_radial_workspace_elems(void);
int nfk_radial_sumsq(const float* x, int64_t ldx, const float* x0, int64_t batch, int32_t dim,
                     double* workspace, double* sumsq, nfk_stream_t stream);
int nfk_radial_apply(const float* x, int64_t ldx, const float* x0, const float* log_alpha,
                     const float* beta, const double* sumsq, float* z, int64_t ldz,
                     float* ld_scalar, float* logdet, int32_t logdet_mode, int64_t batch,
                     int32_t dim, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Isotropic normal prior log-density epilogue: the reference's "Normal" prior
 * MultivariateNormal(0, var*I).log_prob (applications/src/setup.py:25-30)
 * combined with the flow log-det as in nf/models.py:34 and :39:
 *   out[b] = -0.5*(D*log(2pi) + sum_i (z_i/scale)^2) - half_log_det
 *            + sign * logdet[b]          (logdet nullable; sign = +1 or -1)
 * scale = the prior's Cholesky diagonal sqrt(var) (its scale_tril), and
 * half_log_det = sum_i log(scale) are passed in as torch evaluates them.
 *   status: nullable; NFK_ST_NAN_Z is OR-ed in when a row of z holds a NaN
 *           (torch validates the prior's argument: ValueError).
 * ------------------------------------------------------------------------- */
int nfk_normal_logprob(const float* z, int64_t ldz, const float* logdet, float* out,
                       int64_t batch, int32_t dim, float scale, float half_log_det,
                       int32_t sign, int32_t* status, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * NSF_AR conditioner features (nf/flows.py:172-173, 183):
 *   feat[b, j] = cos(pi*x[b,j]/B), feat[b, n+j] = sin(pi*x[b,j]/B), j < n
 * ------------------------------------------------------------------------- */
int nfk_trig_features(const float* x, int64_t ldx, float* feat, int64_t ldf, int64_t batch,
                      int32_t n, double B, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused NSF_AR layer (nfk_fused_ar.hip): replaces NSF_AR.forward / inverse
 * (nf/flows.py:176-209) -- every coordinate's conditioner (FCNN(2i, 3K-1,
 * hidden) on the trig features of coordinates < i, flows.py:172-173, 183; the
 * init_param logits for coordinate 0) and its spline, ONE launch per layer.
 *   weights: a DEVICE array of (dim - 1) x 6 pointers, per conditioner
 *     i = 1 .. dim-1 in order {W1 [hidden][2i], b1, W2 [hidden][hidden], b2,
 *     W3 [3K-1][hidden], b3} (nn.Linear weight/bias, contiguous fp32);
 *   pack: nfk_fused_ar_pack_elems() floats, written by nfk_fused_ar_pack();
 *   x: the layer input [batch, dim] (forward: x, inverse: z); out: the output;
 *   logdet: mode 0 none, 1 write, 2 accumulate (the layer's sum over columns
 *     in column order); status: dim words (column i's reference errors: bit
 *     NFK_ST_INSIDE_SEEN when an element is inside [-B, B], NFK_ST_NEG_DISC).
 * Supported shapes: nfk_fused_ar_supported() != 0.
 * ------------------------------------------------------------------------- */
int nfk_fused_ar_supported(int32_t dim, int32_t hidden, int32_t K);
/* The inverse fused too (NSF_AR.inverse, flows.py:191-209)?  0 for the shapes
 * only the streamed forward covers (Polymer.yaml's 2048 coordinates): their
 * inverse runs per column. */
int nfk_fused_ar_inverse_supported(int32_t dim, int32_t hidden, int32_t K);
int64_t nfk_fused_ar_pack_elems(int32_t dim, int32_t hidden, int32_t K);
int nfk_fused_ar_pack(const float* const* weights, const float* init_param, int32_t dim, int32_t hidden,
                      int32_t K, float* pack, nfk_stream_t stream);
int nfk_fused_ar(const float* x, int64_t ldx, const float* pack, int32_t dim, int32_t hidden, int32_t K,
                 double tail_bound, float* out, int64_t ldo, float* logdet, int32_t logdet_mode,
                 int64_t batch, int32_t inverse, int32_t* status, nfk_stream_t stream);
/* The same with a workspace: a forward whose batch is too small to fill the
 * GPU splits the conditioners over workgroups (they are independent given x,
 * flows.py:182-189) when workspace holds nfk_fused_ar_workspace() floats (the
 * per-column log|det| terms, summed in column order: results bitwise those of
 * nfk_fused_ar).  A null or short workspace runs unsplit; 0 = none needed.
 * The shapes only the streamed forward covers (nfk_fused_ar_inverse_supported()
 * == 0) always need it: it also holds their trig operands. */
int64_t nfk_fused_ar_workspace(int32_t dim, int32_t hidden, int32_t K, int64_t batch, int32_t inverse);
int nfk_fused_ar_ws(const float* x, int64_t ldx, const float* pack, int32_t dim, int32_t hidden, int32_t K,
                    double tail_bound, float* out, int64_t ldo, float* logdet, int32_t logdet_mode,
                    int64_t batch, int32_t inverse, int32_t* status, float* workspace, int64_t workspace_floats,
                    nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused NSF coupling layer: conditioner MLP (FCNN, flows.py:20-35) on MFMA
 * (fp16 two-way split with power-of-two pre-scaling, fp32 accumulation) +
 * spline epilogue, one launch per layer; the [batch, n_up, 3K-1] conditioner
 * output never touches HBM.  Replaces NSF_CL.forward/inverse (flows.py:227-253).
 *   wpack: weights re-packed by nfk_fused_nsf_pack() into MFMA fragment order
 *   (a device buffer of nfk_fused_nsf_pack_elems() floats).
 * Supported shapes: nfk_fused_nsf_supported() != 0.
 * ------------------------------------------------------------------------- */
int nfk_fused_nsf_supported(int32_t n_lo, int32_t n_up, int32_t hidden, int32_t K);
int64_t nfk_fused_nsf_pack_elems(int32_t n_lo, int32_t n_up, int32_t hidden, int32_t K);
int nfk_fused_nsf_pack(const float* w0, const float* b0, const float* w2, const float* b2,
                       const float* w4, const float* b4, int32_t n_lo, int32_t n_up,
                       int32_t hidden, int32_t K, float* wpack, nfk_stream_t stream);
int nfk_fused_nsf(const float* x, int64_t ldx, const float* wpack, const int32_t* up_in,
                  const int32_t* up_out, int32_t n_up, const int32_t* lo_in,
                  const int32_t* lo_out, int32_t n_lo, int32_t hidden, float* z, int64_t ldz,
                  float* logdet, int32_t logdet_mode, int64_t batch, int32_t K,
                  double tail_bound, int32_t inverse, int32_t* status, nfk_stream_t stream);
/* The same with a workspace of nfk_fused_nsf_workspace() floats: layers with a
 * conditioner wider than the instanced NSF_CL kernels (the applications'
 * H = 354, K = 32, setup.py:59-62) split their upper coordinates over
 * workgroups when the batch alone cannot fill the GPU, the per-coordinate
 * log|det| terms going through the workspace (summed in coordinate order:
 * bitwise the unsplit result).  0 floats = no split for this call. */
int64_t nfk_fused_nsf_workspace(int32_t n_lo, int32_t n_up, int32_t hidden, int32_t K, int64_t batch,
                                int32_t inverse);
int nfk_fused_nsf_ws(const float* x, int64_t ldx, const float* wpack, const int32_t* up_in,
                     const int32_t* up_out, int32_t n_up, const int32_t* lo_in, const int32_t* lo_out,
                     int32_t n_lo, int32_t hidden, float* z, int64_t ldz, float* logdet,
                     int32_t logdet_mode, int64_t batch, int32_t K, double tail_bound, int32_t inverse,
                     int32_t* status, float* workspace, int64_t workspace_floats, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Chain of fused NSF coupling layers in one launch: the layer loop of
 * NormalizingFlowModel.forward/inverse (nf/models.py:13-29) over nlayers
 * consecutive NSF_CL layers of one shape (n_lo, n_up, hidden, K, tail_bound)
 * and one direction.  Each wave keeps its 16 x rows in LDS from the first
 * layer to the last: HBM sees x once, z once and log|det| once per chain.
 * Results are bitwise those of nlayers nfk_fused_nsf launches (log|det| is
 * added layer by layer in the same order).
 *   wpacks: DEVICE array of nlayers pack pointers (nfk_fused_nsf_pack), in
 *           execution order.
 *   cmaps:  DEVICE int32 [nlayers * D + D], D = n_lo + n_up: for layer l,
 *           the tile columns of its lower inputs (n_lo) then of its upper
 *           inputs (n_up) -- the layer's lo_in/up_in composed with the column
 *           permutation of the layers before it (the tile keeps x's column
 *           order; a layer overwrites its upper columns in place) -- then, for
 *           every output column o of the last layer, the tile column holding it.
 *   status: nlayers words, one per layer (bits as nfk_rqs_coupling).
 *   log_prob: optional prior epilogue (NormalizingFlowModel.evaluate,
 *           models.py:37-40, Normal prior N(0, s^2 I), setup.py:25-30):
 *           log_prob[b] = log N(z_b; 0, prior_scale^2 I) + log|det|_b with
 *           prior_half_log_det = sum log(scale_tril diagonal) as torch has it
 *           (the constants of nfk_normal_logprob).  With log_prob given, z may
 *           be NULL (not written) and logdet NULL with logdet_mode 0; a NaN in
 *           z ORs NFK_ST_NAN_Z into status[0].
 * nlayers <= nfk_fused_nsf_chain_max() (0: shape not supported by the chain
 * form); x, z 16-byte aligned with ldx, ldz multiples of 4.
 * ------------------------------------------------------------------------- */
int nfk_fused_nsf_chain_max(int32_t n_lo, int32_t n_up, int32_t hidden, int32_t K);
int nfk_fused_nsf_chain(const float* x, int64_t ldx, const float* const* wpacks,
                        const int32_t* cmaps, int32_t nlayers, int32_t n_lo, int32_t n_up,
                        int32_t hidden, float* z, int64_t ldz, float* logdet,
                        int32_t logdet_mode, int64_t batch, int32_t K, double tail_bound,
                        int32_t inverse, int32_t* status, float* log_prob, float prior_scale,
                        float prior_half_log_det, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Training forward of a chain of fused NSF_CL layers (forward direction, the
 * two-tile chain's shapes: nfk_fused_nsf_chain_saved_ok != 0, nlayers >= 2):
 * nfk_fused_nsf_chain's z and log|det|, and in the same launch the INPUT of
 * every layer l >= 1 -- what that layer's backward needs (the per-layer
 * autograd node saves it, nf/models.py:13-20 run under autograd) -- written to
 * saves + (l - 1) * save_stride, rows of ld_saves floats, in that layer's own
 * column order (bitwise the z of layer l - 1).
 *   smaps: DEVICE int32 [(nlayers - 1) * D]: for layer l >= 1 and each of its
 *          input columns, the tile column holding it (the permutation the
 *          chain's cmaps compose at the start of layer l).
 * x, z, saves 16-byte aligned; ldx, ldz, ld_saves, save_stride multiples of 4;
 * D = n_lo + n_up a multiple of 4.
 * ------------------------------------------------------------------------- */
int nfk_fused_nsf_chain_saved_ok(int32_t n_lo, int32_t n_up, int32_t hidden, int32_t K, int32_t nlayers);
int nfk_fused_nsf_chain_saved(const float* x, int64_t ldx, const float* const* wpacks,
                              const int32_t* cmaps, int32_t nlayers, int32_t n_lo, int32_t n_up,
                              int32_t hidden, float* z, int64_t ldz, float* logdet,
                              int32_t logdet_mode, int64_t batch, int32_t K, double tail_bound,
                              int32_t* status, float* saves, int64_t ld_saves, int64_t save_stride,
                              const int32_t* smaps, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Training backward of one fused NSF_CL layer (the VJP of flows.py:227-253,
 * utils.py:58-152 at the layer input x): the conditioner recomputed on the
 * matrix cores as nfk_fused_nsf computes it, and the spline VJP of every
 * element on the logits in registers.  Writes
 *   gparams [batch, n_up, 3K-1]: dL/d(conditioner output), the input of the
 *            conditioner's own backward (GEMMs outside);
 *   gx [batch, D]: upper coordinates dL/dx through the spline, lower ones the
 *            identity part (gz of their output column; the conditioner's part
 *            is added by the caller);
 *   h1, h2 [batch, ldh]: the two tanh activations in columns [0, hidden) and
 *            1.0 at column hidden (ldh >= hidden + 1, a multiple of 4; rows
 *            16-byte aligned), for the weight-gradient GEMMs.
 * gz (dL/dz, [batch, D]) and glogdet (dL/dlog|det|, [batch]) are nullable.
 * vpack: nfk_fused_nsf_vjp_pack (the pack's records in 8-coordinate chunks and
 * their sub-record stream).  Supported: nfk_fused_nsf_vjp_pack_elems() > 0
 * (n_lo <= 32, D <= 128 and a multiple of 4; (KBH, tail, K) instantiated).
 * ------------------------------------------------------------------------- */
int64_t nfk_fused_nsf_vjp_pack_elems(int32_t n_lo, int32_t n_up, int32_t hidden, int32_t K);
int nfk_fused_nsf_vjp_pack(const float* w0, const float* b0, const float* w2, const float* b2,
                           const float* w4, const float* b4, int32_t n_lo, int32_t n_up,
                           int32_t hidden, int32_t K, float* vpack, nfk_stream_t stream);
int nfk_fused_nsf_vjp(const float* x, int64_t ldx, const float* vpack, const int32_t* up_in,
                      const int32_t* up_out, int32_t n_up, const int32_t* lo_in,
                      const int32_t* lo_out, int32_t n_lo, int32_t hidden, const float* gz,
                      int64_t ldgz, const float* glogdet, float* gparams, float* gx, int64_t ldgx,
                      float* h1, float* h2, int64_t ldh, int64_t batch, int32_t K,
                      double tail_bound, int32_t inverse, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Fused RealNVP layer: both affine half-couplings with their four FCNN
 * conditioners (s1, t1, s2, t2) in one launch; replaces RealNVP.forward /
 * inverse (flows.py:44-76).  x, z: [batch, 2*half_dim] row-major.
 *   nets: HOST array of 24 device pointers, nets s1, t1, s2, t2 in that order,
 *         each W0 [H, half_dim], b0, W2 [H, H], b2, W4 [half_dim, H], b4
 *         (nn.Linear weight/bias of network.0/.2/.4).
 * Supported shapes: nfk_fused_realnvp_supported() != 0 (half_dim = 16, 32,
 * 48 or 64; hidden <= 132).
 * ------------------------------------------------------------------------- */
int nfk_fused_realnvp_supported(int32_t half_dim, int32_t hidden);
int64_t nfk_fused_realnvp_pack_elems(int32_t half_dim, int32_t hidden);
int nfk_fused_realnvp_pack(const float* const* nets, int32_t half_dim, int32_t hidden, float* wpack,
                           nfk_stream_t stream);
int nfk_fused_realnvp(const float* x, int64_t ldx, const float* wpack, int32_t half_dim, int32_t hidden,
                      float* z, int64_t ldz, float* logdet, int32_t logdet_mode, int64_t batch,
                      int32_t inverse, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Chained RealNVP layers: nlayers consecutive RealNVP layers of one shape in
 * ONE launch (NormalizingFlowModel's layer loop, models.py:13-20 / 22-29 /
 * 37-40, over RealNVP.forward / inverse, flows.py:52-76).  Each layer's x is
 * the previous layer's z (the lower/upper halves keep their positions), so x
 * rows stay in LDS from the first layer to the last; z and log|det| are
 * bitwise those of nlayers nfk_fused_realnvp launches in the same order.
 *   wpacks: DEVICE array of nlayers pack pointers (nfk_fused_realnvp_pack:
 *           where nfk_fused_realnvp_chain_max() != 0 the pack also holds the
 *           chain's weight stream), in execution order (reversed layer order
 *           when inverse != 0, as the caller runs them).
 *   z: [batch, 2*half_dim] or NULL when log_prob is given.
 *   log_prob: nullable; the isotropic-Normal prior epilogue (the reference's
 *           "Normal" prior, applications/src/setup.py:25-30): log_prob[b] =
 *           log N(z_b; 0, prior_scale^2 I) + log|det|_b (prior_half_log_det =
 *           Sigma log of the scale_tril diagonal), and a NaN in z ORs
 *           NFK_ST_NAN_Z into status[0] (nullable).
 *   x, z rows 16-byte aligned (ldx, ldz multiples of 4).
 * nfk_fused_realnvp_chain_max(): most layers per launch (0: the chain form
 * does not apply to this shape; use nfk_fused_realnvp per layer).
 * ------------------------------------------------------------------------- */
int nfk_fused_realnvp_chain_max(int32_t half_dim, int32_t hidden);
int nfk_fused_realnvp_chain(const float* x, int64_t ldx, const float* const* wpacks, int32_t nlayers,
                            int32_t half_dim, int32_t hidden, float* z, int64_t ldz, float* logdet,
                            int32_t logdet_mode, int64_t batch, int32_t inverse, int32_t* status,
                            float* log_prob, float prior_scale, float prior_half_log_det,
                            nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Training backward of the remaining flow classes (nfk_flows_bwd.hip): the
 * vector-Jacobian products autograd takes through flows_1.py's Planar
 * (:42-60), Radial (:85-97), ActNorm (:207-215), MAF (:171-195) and NSF_AR's
 * trig features (flows.py:172-173).  Batch sums (parameter gradients) are
 * deterministic (fixed-order fp64 column reductions, no atomics).
 *   workspace: device scratch of nfk_flows_bwd_workspace_bytes(batch, dim)
 *              bytes, 256-byte aligned (MAF: dim = 2).
 * Upstream gradients gz (dL/dz) and glogdet (dL/dlog|det|: [batch] per
 * sample, or a [1] scalar where the layer's log|det| is a scalar) are nullable.
 *
 * nfk_planar_bwd: gx [batch, dim]; gw, gu [dim], gb [1] (through the tanh
 *   re-parameterisation of u, flows_1.py:48-53).
 * nfk_actnorm_bwd: gx, gmu, gls (log|det| = +-sum(log_sigma): gld_scalar).
 * nfk_radial_bwd_scalars / _apply: two calls like the forward, because
 *   r = ||x - x0||_F is batch-global: scal[4] = [dL/dsumsq, dL/dlog_alpha,
 *   dL/dbeta, beta_hat h]; a sharded batch all-reduces (sums) scal[0] between
 *   the calls (the backward of the forward's all-reduce of sumsq); _apply
 *   writes gx and g_x0 [dim] (same workspace).
 * nfk_maf_bwd: columns [c0, c1) of nfk_maf with gout = dL/dout: gx at each
 *   column's input position (written), gparams (dL/d conditioner output, the
 *   layout of params), ginit [2] (= the batch sum, written when c0 == 0).
 *   The conditioners' own backward is the caller's (it adds into gx / gout).
 * nfk_trig_features_bwd: gx[:, :n] += dL/dx through nfk_trig_features.
 * ------------------------------------------------------------------------- */
int64_t nfk_flows_bwd_workspace_bytes(int64_t batch, int32_t dim);
int nfk_planar_bwd(const float* x, int64_t ldx, const float* w, const float* u, const float* b,
                   const float* gz, int64_t ldgz, const float* glogdet, float* gx, int64_t ldgx,
                   float* gw, float* gu, float* gb, void* workspace, int64_t batch, int32_t dim,
                   int32_t nonlinearity, nfk_stream_t stream);
int nfk_actnorm_bwd(const float* x, int64_t ldx, const float* mu, const float* log_sigma, int32_t dim,
                    const float* gz, int64_t ldgz, const float* gld_scalar, float* gx, int64_t ldgx,
                    float* gmu, float* gls, void* workspace, int64_t batch, int32_t inverse,
                    nfk_stream_t stream);
int nfk_radial_bwd_scalars(const float* x, int64_t ldx, const float* x0, const float* log_alpha,
                           const float* beta, const double* sumsq, const float* gz, int64_t ldgz,
                           const float* gld_scalar, float* scal, void* workspace, int64_t batch,
                           int32_t dim, nfk_stream_t stream);
int nfk_radial_bwd_apply(const float* x, int64_t ldx, const float* x0, const float* gz, int64_t ldgz,
                         const float* scal, float* gx, int64_t ldgx, float* gx0, void* workspace,
                         int64_t batch, int32_t dim, nfk_stream_t stream);
int nfk_maf_bwd(const float* x, int64_t ldx, const float* init_param, const float* params, int64_t ldp,
                const float* gout, int64_t ldgo, const float* glogdet, int32_t c0, int32_t c1,
                int32_t dim, float* gx, int64_t ldgx, float* gparams, int64_t ldgp, float* ginit,
                void* workspace, int64_t batch, int32_t inverse, nfk_stream_t stream);
int nfk_trig_features_bwd(const float* x, int64_t ldx, const float* gfeat, int64_t ldgf, float* gx,
                          int64_t ldgx, int64_t batch, int32_t n, double B, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Input-gradient GEMMs of the FCNN conditioner's backward (nfk_fcnn_bwd.hip;
 * the dX chain of flows.py:20-35 differentiated), tanh's backward fused:
 *   out[b, j] = (sum_p g[b, p] W[p, j]) * (1 - h[b, j]^2)    (h NULL: no factor)
 * W [P, H] row-major (an nn.Linear weight, out x in) re-packed once by
 * nfk_fcnn_dh_pack into nfk_fcnn_dh_pack_floats(P, H) floats (0: unsupported:
 * P a multiple of 4, H <= 128).  fp16 two-way split on the matrix cores, fp32
 * accumulation, per-row power-of-two scaling of g.  g rows 16-byte aligned.
 * out element (b, j) is out[b*ldo + j*out_col_stride]; accumulate != 0 adds
 * to it (e.g. the lower columns of a layer's dL/dx, written in place).
 * ------------------------------------------------------------------------- */
int64_t nfk_fcnn_dh_pack_floats(int32_t P, int32_t H);
/* [x[:, cols] | 1] for a weight gradient that carries its bias gradient in
 * the last column (the bias of flows.py:26's first nn.Linear):
 *   out[b, j] = x[b*ldx + cols[j]] (j < n), out[b, n] = 1, out[b, n+1 .. ldo) = 0
 * ldo a multiple of 4 and >= n + 1, out 16-byte aligned. */
int nfk_gather_cols_ones(const float* x, int64_t ldx, const int32_t* cols, int32_t n, int64_t batch,
                         float* out, int64_t ldo, nfk_stream_t stream);
int nfk_fcnn_dh_pack(const float* W, int32_t P, int32_t H, float* pack, nfk_stream_t stream);
int nfk_fcnn_dh(const float* g, int64_t ldg, int32_t P, const float* pack, const float* h, int64_t ldh,
                int32_t H, float* out, int64_t ldo, int64_t out_col_stride, int32_t accumulate,
                int64_t batch, nfk_stream_t stream);
/* The same kernel in forward form, for the training recompute of one FCNN
 * Linear (flows.py:26-31, nn.Linear + optional nn.Tanh):
 *   out[b, j] = act(sum_p x[b, p] W[p, j] + bias[j])   act = tanh if tanh_out
 * W [P, H] is the nn.Linear weight TRANSPOSED (in x out), packed by
 * nfk_fcnn_dh_pack; bias may be NULL.  x rows 16-byte aligned, out dense rows. */
int nfk_fcnn_linear(const float* x, int64_t ldx, int32_t P, const float* pack, const float* bias,
                    int32_t tanh_out, int32_t H, float* out, int64_t ldo, int64_t batch,
                    nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * RealNVP layers with wide conditioners at small batches (nfk_wide_rnvp.hip):
 * applications/input/Polymer_rnvp.yaml's RealNVP(2048, hidden 4000) at the
 * config's 40 rows and the driver's sample(100) (applications/examples/
 * polymer.py:29,37-41).  Replaces RealNVP.forward / inverse (nf/flows.py:52-76)
 * with its four FCNN conditioners (flows.py:20-35) when the layer is the
 * weight stream: every weight read once per layer.
 *
 * nfk_wlin_pack: an nn.Linear weight W [N, K] (out x in, row-major) re-packed
 * once into nfk_wlin_pack_floats(N, K) floats (fp16 hi/lo MFMA fragments of
 * 2^s W, one power of two per matrix).
 *
 * nfk_wide_rnvp: one RealNVP layer.  packs / biases: 12 device pointers each,
 * [6 c + 2 l + g] for half-coupling c (0: s1/t1, 1: s2/t2), Linear l (0, 1, 2
 * = network.0, .2, .4) and conditioner g (0 = s, 1 = t); biases are the
 * Linears' fp32 bias vectors.  x [batch, 2 half] (row stride ldx) -> z (ldz;
 * may equal x), logdet mode 0 none / 1 write / 2 accumulate (forward +sum s,
 * inverse -sum s, flows.py:61-62, 74-75).  workspace: at least
 * nfk_wide_rnvp_workspace(half, hidden, batch) floats, 16-byte aligned.  Rows
 * are processed 128 per pass (every pass streams the weights once).
 * half and hidden multiples of 4 (nfk_wide_rnvp_supported).
 * ------------------------------------------------------------------------- */
int64_t nfk_wlin_pack_floats(int32_t N, int32_t K);
int nfk_wlin_pack(const float* W, int32_t N, int32_t K, float* pack, nfk_stream_t stream);
int nfk_wide_rnvp_supported(int32_t half, int32_t hidden);
int64_t nfk_wide_rnvp_workspace(int32_t half, int32_t hidden, int64_t batch);
int nfk_wide_rnvp(const float* x, int64_t ldx, const float* const* packs, const float* const* biases, int32_t half,
                  int32_t hidden, float* z, int64_t ldz, float* logdet, int32_t logdet_mode, int64_t batch,
                  int32_t inverse, float* workspace, int64_t workspace_floats, nfk_stream_t stream);
/* nfk_wide_rnvp_chain: nlayers consecutive such layers in ONE call (the
 * model's layer loop, nf/models.py:13-29 / 22-35, over RealNVP layers of one
 * shape): packs / biases hold 12 pointers per layer in EXECUTION order (the
 * inverse's caller passes the layers last to first).  Bitwise the per-layer
 * calls; the last half-coupling of each layer also writes the next layer's
 * input fragments, so only the first layer converts x.  workspace:
 * nfk_wide_rnvp_chain_workspace(half, hidden, batch) floats. */
int64_t nfk_wide_rnvp_chain_workspace(int32_t half, int32_t hidden, int64_t batch);
int nfk_wide_rnvp_chain(const float* x, int64_t ldx, const float* const* packs, const float* const* biases,
                        int32_t nlayers, int32_t half, int32_t hidden, float* z, int64_t ldz, float* logdet,
                        int32_t logdet_mode, int64_t batch, int32_t inverse, float* workspace,
                        int64_t workspace_floats, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * NSF_AR inverse for the layers the fused kernel's inverse does not take
 * (nfk_fused_ar_inverse_supported == 0: Polymer.yaml's 2,048 coordinates),
 * nfk_ar_seqinv.hip: NSF_AR.inverse (nf/flows.py:193-209) column by column,
 * one launch per coordinate issued from the library (per row, one workgroup
 * finishes conditioner i: its layer-1 partial sums plus x_{i-1}'s two
 * features, layers 2-3, the spline's inverse and the trig features of x_i;
 * beside them, workgroups run conditioner i+1's layer 1 over the features
 * already known, 64 at a time), fp32 arithmetic, the weights read in
 * place.  weights: a HOST array of 6 (dim - 1) device pointers (W1, b1, W2,
 * b2, W3, b3 of conditioners 1 .. dim-1, fp32 contiguous nn.Linear tensors: the
 * entries of the table nfk_fused_ar_pack reads; each launch takes its
 * conditioners' pointers as arguments); init_param [3K-1].  z -> x [batch, dim],
 * logdet mode 0/1/2 (the inverse's -log|det|), status [dim] (nullable).
 * workspace: nfk_ar_seqinv_workspace(dim, hidden, K, batch) floats.  64 rows
 * per pass.  hidden <= 128, K in {4, 8, 10, 16, 32}.
 * ------------------------------------------------------------------------- */
int nfk_ar_seqinv_supported(int32_t dim, int32_t hidden, int32_t K);
int64_t nfk_ar_seqinv_workspace(int32_t dim, int32_t hidden, int32_t K, int64_t batch);
int nfk_ar_seqinv(const float* z, int64_t ldz, const float* const* weights, const float* init_param, int32_t dim,
                  int32_t hidden, int32_t K, double tail_bound, float* x, int64_t ldx, float* logdet,
                  int32_t logdet_mode, int64_t batch, int32_t* status, float* workspace, int64_t workspace_floats,
                  nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Priors and targets of the applications layer (applications/src/systems.py),
 * nfk_systems.hip.  No MFMA, no atomics on floats: every sum has a fixed
 * order, so two runs are bitwise equal.
 *
 * Einstein crystal (systems.py:366-372): per row, with D = natoms * dim and
 * centers [natoms, dim] dense,
 *   dev_c = z_c - centers_c;  has_box: dev_c -= (|dev_c| > (float)(0.5 L)) sign(dev_c) (float)L
 *   out[b] = -0.5*(D*log(2pi) + sum_c (dev_c/scale)^2) - natoms*half_log_det
 *            + sign * logdet[b]          (logdet nullable; sign = +1 or -1)
 * scale = sqrt(1/alpha) and half_log_det = dim*log(scale) are those of the
 * per-atom MultivariateNormal(0, I/alpha) as torch evaluates them (the
 * constants of nfk_normal_logprob, per atom).  boxlength is L (a double, as
 * the reference's Python scalar); has_box = 0 skips the wrap.
 *   status: nullable; NFK_ST_NAN_Z is OR-ed in when a row of z holds a NaN.
 * Rows that are 16-byte aligned with D % 4 == 0 take a float4 form
 * (y = dev * (1/scale): <= 1 ulp per element from the scalar form's dev/scale).
 * Backward: gz[b, c] = -dev_c / scale^2 * g[b] (the wrap has zero derivative).
 * ------------------------------------------------------------------------- */
int nfk_einstein_logprob(const float* z, int64_t ldz, const float* centers, const float* logdet,
                         float* out, int64_t batch, int32_t natoms, int32_t dim, float scale,
                         float half_log_det, int32_t has_box, double boxlength, int32_t sign,
                         int32_t* status, nfk_stream_t stream);
int nfk_einstein_logprob_bwd(const float* z, int64_t ldz, const float* centers, const float* g,
                             float* gz, int64_t ldgz, int64_t batch, int32_t natoms, int32_t dim,
                             float scale, int32_t has_box, double boxlength, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Gaussian mixture (systems.py:287-292): a row holds npart particles of dim
 * coordinates; centers [ncenters, dim], scales [ncenters] (sqrt(var_i), the
 * components' Cholesky diagonals) and hlds [ncenters] (dim*log(scale_i)) dense.
 *   p(x)   = sum_i (float)(1/ncenters) * exp(-0.5*(dim*log(2pi) + |(x-c_i)/scale_i|^2) - hld_i)
 *            accumulated in centre order with accurate expf (not a log-sum-exp:
 *            a particle far from every centre gives log(0) = -inf, as the
 *            reference does)
 *   out[b] = sum_particles log p(x) + sign * logdet[b]
 *   status: nullable; NFK_ST_NAN_Z on a NaN row.
 * Backward: gx = g[b] * sum_i p_i * (-(x-c_i)/var_i) / p(x) (NaN where p(x) == 0,
 * as torch's autograd gives).
 * Supported shapes: nfk_gmix_supported() != 0 (ncenters <= 64, dim <= 4).
 * ------------------------------------------------------------------------- */
int nfk_gmix_supported(int32_t ncenters, int32_t dim);
int nfk_gmix_logprob(const float* x, int64_t ldx, const float* centers, const float* scales,
                     const float* hlds, const float* logdet, float* out, int64_t batch,
                     int32_t npart, int32_t dim, int32_t ncenters, int32_t sign, int32_t* status,
                     nfk_stream_t stream);
int nfk_gmix_logprob_bwd(const float* x, int64_t ldx, const float* centers, const float* scales,
                         const float* hlds, const float* g, float* gx, int64_t ldgx, int64_t batch,
                         int32_t npart, int32_t dim, int32_t ncenters, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Lennard-Jones energy of a periodic box (LJ.potential, systems.py:154-189),
 * x [batch, n*dim] rows of n particles, with the reference's arithmetic: per
 * pair (i, j), i != j included twice and the diagonal too,
 *   d_c = x_ic - x_jc;  d_c -= (|d_c| > (float)(0.5 L)) sign(d_c) (float)L   (one wrap)
 *   r = |d|;  inv = 1/(r + (r == 0));  has_cutoff: inv = 0 where r > cutoff
 *   p6 = (sigma*inv)^6;  u = 4 epsilon (p6^2 - p6 [- s6^2 + s6 with has_cutoff and shift,
 *   s6 = (sigma/cutoff)^6]);  u *= inv * r  (zero on the diagonal, for coincident
 *   pairs and beyond the cutoff)
 *   out[b] = sum_ij u / 2
 * n <= 64: a row takes a group of next_pow2(n) lanes (64 / group rows per
 * wave); 64 < n <= 256: one row per wave.  Lane i keeps particle i (and i + 64,
 * ...) in registers and walks j through the row staged in LDS (one broadcast
 * read per j), so no [n, n] temporary exists; the row's energy is a fixed-order
 * sum.  Backward: gx[b, i] = g[b] * sum_j u'(r_ij) d_ij / r_ij (the force on i,
 * negated), each lane summing its own particle: no atomics.
 * Supported shapes: nfk_lj_supported() != 0 (n <= 256, dim 2 or 3).
 * ------------------------------------------------------------------------- */
int nfk_lj_supported(int32_t n, int32_t dim);
int nfk_lj_potential(const float* x, int64_t ldx, float* out, int64_t batch, int32_t n, int32_t dim,
                     double boxlength, double sigma, double epsilon, int32_t has_cutoff,
                     double cutoff, int32_t shift, nfk_stream_t stream);
int nfk_lj_potential_bwd(const float* x, int64_t ldx, const float* g, float* gx, int64_t ldgx,
                         int64_t batch, int32_t n, int32_t dim, double boxlength, double sigma,
                         double epsilon, int32_t has_cutoff, double cutoff, int32_t shift,
                         nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Embedded-atom energy from setfl tables, nfk_eam.hip (systems.py EAM): n atoms
 * of one species in a periodic orthorhombic box (lx, ly, lz), x [batch, n*3]
 * (row stride ldx) -> out [batch]:
 *   rho_i = sum_(j,s) f(r_ijs)
 *   U     = sum_i F(rho_i) + 1/2 sum_i sum_(j,s) z(r_ijs) / r_ijs
 * s runs over integer image shifts, r_ijs = |x_i - x_j + s*L|, and a term counts
 * when 0 < r_ijs <= rc: EVERY periodic image inside the cutoff, self images
 * (i == j, s != 0) included; only r == 0 is skipped (the atom itself, and a
 * coincident atom).  Each component of x_i - x_j is wrapped once into
 * [-L/2, L/2], v - (float)L * rint(v * (float)(1/L)); then the shifts -n_a..n_a,
 * n_a = floor(rc / L_a + 0.5) (at most 8), are visited per axis, x outermost,
 * ascending, the component being v + (float)s * (float)L.  j is the outer loop.
 * Tables: piecewise cubics, one quadruple (c3, c4, s, y) per interval m with
 * value ((c3 p + c4) p + s) p + y at p = t - m, t = x * (float)(1 / dx), and
 * derivative ((3 c3 p + 2 c4) p + s) * (float)(1 / dx).
 *   rtab [2 (nr - 1)] float4: f's quadruple at [2m], z's (z = r phi) at [2m + 1];
 *     m = min((int)t, nr - 2), p clamped to 1.
 *   ftab [nrho - 1] float4: F's; m = (int)t clamped to [0, nrho - 2], p not
 *     clamped below 0; from rho_max = (nrho - 1) drho on (and for a NaN)
 *     F = f_end + fp_end (rho - rho_max), f_end and fp_end being F and dF/drho
 *     at the last node.
 * Both tables are device pointers, 16-byte aligned.
 * Backward: gx[b, i] = g[b] * sum_(j != i, s) [phi' + (F'(rho_i) + F'(rho_j)) f'] d / r
 * with phi = z / r and phi' = (z' - phi) / r: the exact gradient of the
 * interpolated energy (self images do not depend on x_i).
 * Layout as nfk_lj_potential (a row on next_pow2(n) <= 64 lanes, up to 4 atoms
 * per lane, the row staged in LDS as float4); fixed-order sums, no atomics;
 * the backward leaves F'(rho_j) beside x_j in LDS between its two (j, s) loops.
 * Supported shapes: nfk_eam_supported() != 0 (n <= 256).  nr or nrho < 2, a
 * spacing, box length or cutoff <= 0, rc / L_a > 8, misaligned tables:
 * NFK_EINVAL, nothing launched.
 * ------------------------------------------------------------------------- */
int nfk_eam_supported(int32_t n);
int nfk_eam_potential(const float* x, int64_t ldx, float* out, int64_t batch, int32_t n,
                      const float* rtab, int32_t nr, double dr, const float* ftab, int32_t nrho,
                      double drho, double f_end, double fp_end, double lx, double ly, double lz,
                      double rc, nfk_stream_t stream);
int nfk_eam_potential_bwd(const float* x, int64_t ldx, const float* g, float* gx, int64_t ldgx,
                          int64_t batch, int32_t n, const float* rtab, int32_t nr, double dr,
                          const float* ftab, int32_t nrho, double drho, double f_end, double fp_end,
                          double lx, double ly, double lz, double rc, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Dynamics of the three systems, nfk_dynamics.hip: integration_step
 * (systems.py:297-338, 382-401) for a batch of independent trajectories in ONE
 * launch, and the Metropolis step of HMC (nf/hmc.py:56-63).
 *
 * x_in, v_in [batch, W] (row strides ldxi, ldvi; W = natoms*dim, npart*dim or
 * n*dim) -> x_out, v_out (ldxo, ldvo; x_out may be x_in and v_out may be v_in,
 * with the same stride) and pot_out [batch], the potential at x_out: -log_prob
 * for the Einstein crystal and the mixture, the energy for Lennard-Jones, with
 * the arithmetic of nfk_einstein_logprob (its scalar form) / nfk_gmix_logprob /
 * nfk_lj_potential.  All fp32, no contraction.  dt and dt_sq are the
 * reference's Python scalars dt and dt**2, rounded to fp32 once on the host.
 * With G = F(x_in), per step, path_len (>= 0) times, in this order:
 *   x' = (x + v*dt) + (G*0.5f)*dt_sq
 *   Gn = F(scheme ? x' : x)
 *   v' = v + (dt*(G + Gn))*0.5f;   x = x', v = v', G = Gn
 * scheme 0 is the reference's integrator, which evaluates the "new" force at
 * the OLD position (G_k = F(x_{k-1}): not time-reversible); scheme 1 is
 * velocity Verlet (G_k = F(x_k)).  path_len = 0 copies x and v and returns the
 * potential.  F = -dU/dx is the expression of the system's backward entry
 * point at g = 1, the same device functions in the same order: d log_prob/dx
 * of nfk_einstein_logprob_bwd / nfk_gmix_logprob_bwd, the negated gx of
 * nfk_lj_potential_bwd.  So a launch equals, bit for bit in x and v, the chain
 * of those kernels and elementwise fp32 ops it replaces.  NaN and inf
 * propagate as they do there; there is no status word.
 * x, v and the current force stay in registers across the step loop (a
 * wave-uniform runtime bound).  Einstein: a lane per coordinate; mixture: a
 * lane per particle (both forces act on their own coordinate / particle alone,
 * so a lane finishes one trajectory and takes the next, lanes_for(W) further
 * on); the row potential is the fixed-order group sum of the log-density
 * kernels.  Lennard-Jones: nfk_lj_potential's mapping (a row on next_pow2(n)
 * lanes for n <= 64, a wave with up to 4 particles per lane for n <= 256);
 * every step re-stages the row's positions in LDS as float4 and the j loop
 * reads them by broadcast; two LDS buffers per row (<= 32 KiB per block) leave
 * one barrier per step.  Grid-stride over rows with the grid caps of the
 * kernels they follow.
 * The system constants are those of nfk_einstein_logprob / nfk_gmix_logprob /
 * nfk_lj_potential, and so are the supported shapes (nfk_gmix_supported,
 * nfk_lj_supported).  scheme outside {0, 1}, path_len < 0, a leading dimension
 * below W or an unsupported shape: NFK_EINVAL, and nothing is launched.
 * ------------------------------------------------------------------------- */
int nfk_einstein_trajectory(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                            float* x_out, int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out,
                            int64_t batch, int32_t path_len, double dt, double dt_sq, int32_t scheme,
                            const float* centers, int32_t natoms, int32_t dim, float scale,
                            float half_log_det, int32_t has_box, double boxlength, nfk_stream_t stream);
int nfk_gmix_trajectory(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi,
                        float* x_out, int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out,
                        int64_t batch, int32_t path_len, double dt, double dt_sq, int32_t scheme,
                        const float* centers, const float* scales, const float* hlds, int32_t npart,
                        int32_t dim, int32_t ncenters, nfk_stream_t stream);
int nfk_lj_trajectory(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                      int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out, int64_t batch,
                      int32_t path_len, double dt, double dt_sq, int32_t scheme, int32_t n, int32_t dim,
                      double boxlength, double sigma, double epsilon, int32_t has_cutoff, double cutoff,
                      int32_t shift, nfk_stream_t stream);
/* nfk_eam_trajectory: the same contract for the embedded-atom model, rows of
 * W = n*3.  Trajectory arguments as nfk_lj_trajectory, table and box arguments
 * as nfk_eam_potential.  F = -(1.0f * gx) with gx of nfk_eam_potential_bwd at
 * g = 1 and pot_out is nfk_eam_potential at x_out, the same device functions
 * (nfk_systems_dev.h) in nfk_eam_potential's mapping and summation order: a
 * launch equals, bit for bit in x, v AND pot_out, the chain of those kernels and
 * elementwise fp32 ops it replaces.  x, v and the current force stay in
 * registers; two LDS buffers per row (<= 32 KiB per block).  A force evaluation
 * on a staged row is nfk_eam_potential_bwd's two (j, s) loops with F'(rho_j)
 * left beside x_j in LDS and a barrier between them, so a step costs two
 * barriers; all of them sit in block-uniform control flow.  Grid-stride over
 * rows, at most 16,384 blocks.  Supported shapes: nfk_eam_supported(n).
 * NFK_EINVAL, nothing launched: what nfk_lj_trajectory and nfk_eam_potential
 * refuse. */
int nfk_eam_trajectory(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                       int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out, int64_t batch,
                       int32_t path_len, double dt, double dt_sq, int32_t scheme, int32_t n,
                       const float* rtab, int32_t nr, double dr, const float* ftab, int32_t nrho,
                       double drho, double f_end, double fp_end, double lx, double ly, double lz,
                       double rc, nfk_stream_t stream);
/* nfk_hmc_accept: chain c of `chains` accepts its proposal when
 *   r[c] < expf(((u_cur[c] - u_new[c]) [+ k_cur[c]) - k_new[c]] * (float)beta)
 * (accurate expf; k_cur and k_new are both null -- the reference's
 * potential-only test -- or both given; a NaN exponent compares false: a
 * rejection).  On acceptance x_cur[c, :width] = x_new[c, :width],
 * u_cur[c] = u_new[c] and naccept[c] += 1 (int32, nullable); a rejected chain
 * is left as it is.  x_cur (row stride ldc) and x_new (ldn) do not overlap.  A
 * chain takes next_pow2(width) <= 64 lanes whose first lane decides; all
 * writes are ordinary vector stores. */
int nfk_hmc_accept(float* x_cur, int64_t ldc, const float* x_new, int64_t ldn, float* u_cur,
                   const float* u_new, const float* k_cur, const float* k_new, const float* r,
                   int32_t* naccept, int64_t chains, int32_t width, double beta, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Whole HMC runs, nfk_hmc_run.hip: `epochs` moves of `chains` independent
 * chains (nf/hmc.py:50-63) in ONE launch.  The random numbers are read, not
 * made: v_draws [epochs, chains, W] dense holds the velocity draws, already
 * scaled by sqrt(var), and r [epochs, chains] the uniforms.  Per chain c, with
 * x = x_cur[c, :W] (row stride ldx) and u = u_cur[c] in registers, epoch e is
 *   pos_rec[e, c, :] = x, pot_rec[e, c] = u      (both given or both null:
 *                                                 entry e is the state BEFORE move e)
 *   (x', v', u') = the system's nfk_*_trajectory from (x, v_draws[e, c, :]):
 *                  path_len steps of the text above, the same device functions
 *                  (step_x / step_v of nfk_step.h, the forces and the closing
 *                  potential of nfk_systems_dev.h), the same group-sum tree, no
 *                  contraction -- bit for bit that launch's x_out, v_out, pot_out
 *   d = u - u';  hamiltonian: d = (d + k) - k'
 *   accept iff r[e, c] < expf(d * (float)beta)    (nfk_hmc_accept's test; a NaN rejects)
 *   accepted: x = x', u = u', count += 1
 * and afterwards x_cur[c, :] = x, u_cur[c] = u, naccept[c] += count (int32,
 * nullable) and v_last[c, :W] (row stride ldv, nullable) = the v' of the LAST
 * epoch, accepted or not.  So without `hamiltonian` a run equals, bit for bit,
 * `epochs` pairs of nfk_*_trajectory and nfk_hmc_accept launches fed the same
 * draws.  With `hamiltonian` the kinetic energies are computed here, k from
 * the draw and k' from v': each lane sums v*v over its own elements in
 * ascending order, the lanes of the chain are summed by the group-sum
 * butterfly, and the sum is multiplied by 0.5f.  This is the one place where
 * the bits may differ from the per-epoch chain of launches, whose K is a torch
 * row reduction in another order.
 * Mapping (the trajectory kernels', with the chain's state on chip across the
 * epochs): Einstein -- a chain on next_pow2(D) <= 64 lanes, up to 8 coordinates
 * per lane (D = natoms*dim <= 512); mixture -- a particle per lane, up to 4 per
 * lane (npart <= 256, nfk_gmix_supported); Lennard-Jones -- nfk_lj_trajectory's
 * mapping (nfk_lj_supported), x in registers, the row staged in two LDS
 * buffers, restaged from x after every decision whatever it was, so that every
 * barrier sits in block-uniform control flow; rows past `chains` walk the
 * barriers without touching memory.  The chain's first lane decides and
 * broadcasts the decision.  Plain vector stores, no atomics, nothing between
 * workgroups.  x_cur, v_last and the records do not overlap each other or the
 * draws.
 * The *_hmc_supported queries are host-only.  NFK_EINVAL, nothing launched:
 * chains, epochs or path_len below zero; scheme outside {0, 1}; an unsupported
 * shape; exactly one of pos_rec / pot_rec; and, with chains > 0 and
 * epochs > 0, a null x_cur / u_cur / v_draws / r (or system parameter), ldx
 * below W, or ldv below W with v_last given.  chains == 0 or epochs == 0
 * returns 0 without a launch.
 * ------------------------------------------------------------------------- */
int nfk_einstein_hmc_supported(int32_t natoms, int32_t dim);
int nfk_gmix_hmc_supported(int32_t npart, int32_t dim, int32_t ncenters);
int nfk_lj_hmc_supported(int32_t n, int32_t dim);
int nfk_einstein_hmc_run(float* x_cur, int64_t ldx, float* u_cur, int32_t* naccept, const float* v_draws,
                         const float* r, float* v_last, int64_t ldv, float* pos_rec, float* pot_rec,
                         int64_t chains, int32_t epochs, int32_t path_len, double dt, double dt_sq,
                         int32_t scheme, double beta, int32_t hamiltonian, const float* centers,
                         int32_t natoms, int32_t dim, float scale, float half_log_det, int32_t has_box,
                         double boxlength, nfk_stream_t stream);
int nfk_gmix_hmc_run(float* x_cur, int64_t ldx, float* u_cur, int32_t* naccept, const float* v_draws,
                     const float* r, float* v_last, int64_t ldv, float* pos_rec, float* pot_rec,
                     int64_t chains, int32_t epochs, int32_t path_len, double dt, double dt_sq,
                     int32_t scheme, double beta, int32_t hamiltonian, const float* centers,
                     const float* scales, const float* hlds, int32_t npart, int32_t dim, int32_t ncenters,
                     nfk_stream_t stream);
int nfk_lj_hmc_run(float* x_cur, int64_t ldx, float* u_cur, int32_t* naccept, const float* v_draws,
                   const float* r, float* v_last, int64_t ldv, float* pos_rec, float* pot_rec,
                   int64_t chains, int32_t epochs, int32_t path_len, double dt, double dt_sq, int32_t scheme,
                   double beta, int32_t hamiltonian, int32_t n, int32_t dim, double boxlength, double sigma,
                   double epsilon, int32_t has_cutoff, double cutoff, int32_t shift, nfk_stream_t stream);
/* nfk_eam_hmc_run: the same contract for the embedded-atom model: an epoch is
 * nfk_eam_trajectory's arithmetic followed by nfk_hmc_accept's test, in
 * nfk_lj_hmc_run's arrangement (x in registers, two LDS buffers per row, the
 * unconditional restage after the decision).  Run arguments as nfk_lj_hmc_run,
 * table and box arguments as nfk_eam_potential, which also names what is
 * refused about them (checked before chains == 0 or epochs == 0 returns).
 * nfk_eam_hmc_supported(n) == nfk_eam_supported(n). */
int nfk_eam_hmc_supported(int32_t n);
int nfk_eam_hmc_run(float* x_cur, int64_t ldx, float* u_cur, int32_t* naccept, const float* v_draws,
                    const float* r, float* v_last, int64_t ldv, float* pos_rec, float* pot_rec,
                    int64_t chains, int32_t epochs, int32_t path_len, double dt, double dt_sq, int32_t scheme,
                    double beta, int32_t hamiltonian, int32_t n, const float* rtab, int32_t nr, double dr,
                    const float* ftab, int32_t nrho, double drho, double f_end, double fp_end, double lx,
                    double ly, double lz, double rc, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Device random numbers, nfk_rng.h / nfk_langevin.hip: Philox4x32-10 with the
 * Random123 constants (multipliers 0xD2511F53, 0xCD9E8D57; Weyl increments
 * 0x9E3779B9, 0xBB67AE85; 10 rounds).  A call is addressed by
 *   counter = (step_lo, step_hi, particle, row),  key = (seed_lo, seed_hi | tag << 31)
 * with `step` the absolute 64-bit step index, row = (uint32)(row_base + b),
 * 0 <= seed < 2^63 and tag 0 (thermostat noise) or 1 (initial velocities): a
 * value never depends on the launch geometry.  The four words w of a call give
 * four normals by two Box-Muller pairs, u = ((w >> 8) + 0.5f) * 2^-24 in fp32,
 * r = sqrtf(-2 logf(u_a)), (z_a, z_b) = r * (cospif, sinpif)(2 u_b) for
 * (a, b) = (0, 1) and (2, 3), accurate functions; |z| <= 5.89.  Component d of
 * particle p is normal d of its call (dim <= 4).  zero_mean subtracts from each
 * normal its dimension's mean over the row's n particles, summed as the row
 * kernels do: a row on lanes_for(n) = next_pow2(n) <= 64 lanes, each lane its
 * own particles c0 + q lanes in ascending order, the fixed butterfly over the
 * lanes, then / (float)n.
 * nfk_philox_fill writes, for rows b < rows and particles p < n, the raw words
 * as int32 [rows, n, 4] (normals == 0) or the normals as fp32 [rows, n, dim]
 * (normals != 0), dense.  NFK_EINVAL, nothing launched: n outside 1..2^24, dim
 * outside 1..4 with normals, tag outside {0, 1}, zero_mean without normals,
 * seed or step below zero (a seed of 2^63 or more), rows < 0, row_base < 0 or
 * row_base + rows above 2^32, a null `out` with rows > 0.
 * ------------------------------------------------------------------------- */
int nfk_philox_fill(void* out, int32_t normals, int64_t rows, int32_t n, int32_t dim, int64_t step,
                    int64_t row_base, int64_t seed, int32_t tag, int32_t zero_mean, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Langevin (NVT) dynamics, nfk_langevin.hip: `nsteps` BAOAB steps of a batch of
 * independent trajectories in ONE launch, the noise generated in the kernel.
 * x_in, v_in, x_out, v_out, pot_out, batch and the system arguments are those
 * of the system's nfk_*_trajectory (x_out may be x_in, v_out may be v_in), and
 * so are the mappings, the LDS arrangement, the forces and the closing
 * potential (nfk_systems_dev.h) and the supported shapes; the Einstein crystal
 * additionally needs dim <= 4 (a lane holds component c % dim of atom c / dim).
 * With F = force(x_in), per step k < nsteps, in fp32 without contraction and in
 * this order:
 *   v = v + hb*F;  x = x + hd*v;  v = c1*v + c2*xi;  x = x + hd*v;
 *   F = force(x);  v = v + hb*F
 * xi = the tag-0 normal of (seed, step0 + k, particle, row_base + b, component)
 * above, less the row mean with zero_mean.  The host computes in double and
 * rounds to fp32 once: hb = 0.5 dt / mass, hd = 0.5 dt, c1 = exp(-gamma dt),
 * c2 = sqrt(kT / mass * (1 - c1^2)).  Positions are not wrapped.  Since the
 * noise is keyed by the absolute step and F is recomputed from x, a run cut
 * into several calls (step0 advanced, x and v carried) or into row blocks
 * (row_base advanced) equals the single call bit for bit, and a call equals,
 * bit for bit in x, v and the potentials, the chain of nfk_philox_fill, force
 * kernels and elementwise fp32 ops it replaces.
 * Records: with record_every > 0 and pos_rec / pot_rec given (both or neither),
 * after every step with (step0 + k + 1) % record_every == 0 the positions go to
 * pos_rec[f, b, :W] and their potential to pot_rec[f, b], dense, f = (step0 + k
 * + 1) / record_every - 1 - step0 / record_every: (step0 + nsteps) /
 * record_every - step0 / record_every frames.  The potential is evaluated only
 * there and at the end.  Plain vector stores, no atomics, nothing between
 * workgroups.  The records overlap nothing else.
 * NFK_EINVAL, nothing launched: what the system's nfk_*_trajectory refuses about
 * its arguments; nsteps, step0 or record_every below zero; exactly one of
 * pos_rec / pot_rec; a seed outside [0, 2^63); row_base < 0 or row_base + batch
 * above 2^32; an unsupported shape.
 * ------------------------------------------------------------------------- */
int nfk_einstein_langevin(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                          int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out, int64_t batch,
                          int32_t nsteps, int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean,
                          float hb, float hd, float c1, float c2, int32_t record_every, float* pos_rec,
                          float* pot_rec, const float* centers, int32_t natoms, int32_t dim, float scale,
                          float half_log_det, int32_t has_box, double boxlength, nfk_stream_t stream);
int nfk_gmix_langevin(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                      int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out, int64_t batch,
                      int32_t nsteps, int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean,
                      float hb, float hd, float c1, float c2, int32_t record_every, float* pos_rec,
                      float* pot_rec, const float* centers, const float* scales, const float* hlds,
                      int32_t npart, int32_t dim, int32_t ncenters, nfk_stream_t stream);
int nfk_lj_langevin(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                    int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out, int64_t batch, int32_t nsteps,
                    int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean, float hb, float hd,
                    float c1, float c2, int32_t record_every, float* pos_rec, float* pot_rec, int32_t n,
                    int32_t dim, double boxlength, double sigma, double epsilon, int32_t has_cutoff,
                    double cutoff, int32_t shift, nfk_stream_t stream);
int nfk_eam_langevin(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out,
                     int64_t ldxo, float* v_out, int64_t ldvo, float* pot_out, int64_t batch, int32_t nsteps,
                     int64_t step0, int64_t row_base, int64_t seed, int32_t zero_mean, float hb, float hd,
                     float c1, float c2, int32_t record_every, float* pos_rec, float* pot_rec, int32_t n,
                     const float* rtab, int32_t nr, double dr, const float* ftab, int32_t nrho, double drho,
                     double f_end, double fp_end, double lx, double ly, double lz, double rc,
                     nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Hamiltonian switching, nfk_switch.hip: `nsteps` BAOAB steps on the mixed
 * reduced potential u_lam = (1 - lam) u_A + lam U_B / kT between an Einstein
 * crystal A (u_A = -log p_A; centers [n, dim], scale, half_log_det, has_box,
 * boxlength_A as nfk_einstein_langevin; natoms_A == n and dim_A == the target's
 * dim) and the target B of nfk_lj_langevin / nfk_eam_langevin, in ONE launch,
 * with the switching work accumulated in fp64.  Mapping, LDS arrangement, noise
 * (tag 0, keyed by seed, absolute step, particle, row), zero_mean, the frame
 * schedule and the supported shapes are those of the target's *_langevin call.
 * lam[j], 0 <= j < lam_len, is the schedule indexed by the ABSOLUTE step;
 * step0 + nsteps < lam_len.  Per step k, l0 = lam[step0+k], l1 = lam[step0+k+1]:
 *   if (l1 != l0)  w = w + ((double)l1 - (double)l0) * ((double)U_B(x) * inv_kT - (double)u_A(x))
 *   a = (1.0f - l1) * kT;  b = l1;  F = a * g_A + b * g_B        (fp32, this order)
 *   v = v + hb*F;  x = x + hd*v;  v = c1*v + c2*xi(step0+k);  x = x + hd*v
 *   g_A = d log p_A/dx, g_B = -dU_B/dx at the new x;  F = a * g_A + b * g_B;  v = v + hb*F
 * w starts from work[b] and is written back there (work: fp64 [batch], may be
 * null), so chunks of a run add in one order.  en_out [batch, 2] receives
 * (u_A, U_B) at x_out; with record_every > 0 and pos_rec / en_rec (both or
 * neither) the frames [F, batch, n*dim] and their energies [F, batch, 2].
 * nsteps == 0 evaluates the energies only (lam may then be null).  U_B has the
 * bits of nfk_lj_potential / nfk_eam_potential; u_A's row sum runs in the
 * kernel's own fixed order (nfk_switch.hip's head comment).
 * NFK_EINVAL, nothing launched: what the target's *_langevin call refuses; a
 * null or too short schedule with nsteps > 0; natoms_A != n; dim_A != dim;
 * scale <= 0; NaN kT or inv_kT; exactly one of pos_rec / en_rec.
 * ------------------------------------------------------------------------- */
int nfk_lj_switch(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out, int64_t ldxo,
                  float* v_out, int64_t ldvo, float* en_out, int64_t batch, int32_t nsteps, int64_t step0,
                  int64_t row_base, int64_t seed, int32_t zero_mean, float hb, float hd, float c1, float c2,
                  int32_t record_every, float* pos_rec, float* en_rec, int32_t n, int32_t dim, double boxlength,
                  double sigma, double epsilon, int32_t has_cutoff, double cutoff, int32_t shift,
                  const float* centers, int32_t natoms_A, int32_t dim_A, float scale, float half_log_det,
                  int32_t has_box, double boxlength_A, const float* lam, int64_t lam_len, double inv_kT,
                  float kT, double* work, nfk_stream_t stream);
int nfk_eam_switch(const float* x_in, int64_t ldxi, const float* v_in, int64_t ldvi, float* x_out, int64_t ldxo,
                   float* v_out, int64_t ldvo, float* en_out, int64_t batch, int32_t nsteps, int64_t step0,
                   int64_t row_base, int64_t seed, int32_t zero_mean, float hb, float hd, float c1, float c2,
                   int32_t record_every, float* pos_rec, float* en_rec, int32_t n, const float* rtab, int32_t nr,
                   double dr, const float* ftab, int32_t nrho, double drho, double f_end, double fp_end,
                   double lx, double ly, double lz, double rc, const float* centers, int32_t natoms_A,
                   int32_t dim_A, float scale, float half_log_det, int32_t has_box, double boxlength_A,
                   const float* lam, int64_t lam_len, double inv_kT, float kT, double* work,
                   nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Bennett acceptance ratio (applications/src/bar.py:16-68), `problems`
 * independent solves in one launch, and the exponential averages of
 * test.py:67-68.  Problem p works on wf_i = w_f[idx_f ? idx_f[p*ldif + i] : i],
 * i < n_f, and wr_i likewise (int32 row gathers, e.g. bootstrap resamples; both
 * null: the plain vectors).  Inputs are fp32, promoted once; all arithmetic is
 * fp64 without contraction.  With M = log(n_f / n_r) and
 * g(a) = -log(1 + e^a), one iteration maps D to
 *   D' = [LSE_i(g(M - wr_i - D) - wr_i) - log n_r] - [LSE_i g(M + wf_i - D) - log n_f]
 * (LSE: max-shifted log-sum-exp; the largest term of either sum is that of the
 * smallest work value, g being non-increasing, so the max pass runs once over
 * the work values and an iteration is one sum pass), starting at delta0.
 * After iteration k
 * (0-based) rc = |(D' - D) / D'|; the loop stops when k > 0 && rc < rtol, or
 * k + 1 == max_iterations, so rtol = 0 returns exactly the max_iterations-th
 * iterate.  iters[p] = iterations done, out[p*3] = the last D',
 * out[p*3+1] = log mean_i exp(wf_i), out[p*3+2] = log mean_i exp(wr_i) (both
 * max-shifted).
 * Deviations from the reference's text: (1) g is evaluated as
 * -(max(a,0) + log1p(exp(-|a|))), finite for every finite a (the reference's
 * form shifts by min(a,0) and overflows for |a| >~ 709; same function,
 * rounding apart); (2) a NaN D' ends the loop at once and is returned (the
 * reference spins to maximum_iterations and returns the same NaN); (3) every
 * loop exit compares one LDS word read by all lanes: the trip count is
 * workgroup-uniform and bounded by max_iterations.
 * One workgroup per problem (256, 512 or 1024 threads by n_f + n_r alone;
 * grid-stride above 4096 problems), no atomics.  n_f + n_r <= nfk_bar_stage_cap(): the work values are gathered
 * once into LDS (fp32) and every pass reads them there; otherwise every pass
 * re-reads them from global memory through the index rows.  Both forms give a
 * lane the same elements in the same order and share one reduction tree: same
 * bits, and two runs are bitwise equal.  Index values are not validated.
 * NFK_EINVAL, nothing launched: n_f < 1, n_r < 1, problems < 1,
 * max_iterations < 1, rtol < 0 or NaN, a leading dimension below its row
 * length, null w_f / w_r / out / iters, exactly one of idx_f / idx_r when
 * problems > 1.
 * ------------------------------------------------------------------------- */
int nfk_bar_stage_cap(void); /* host-only: largest n_f + n_r kept in LDS */
int nfk_bar(const float* w_f, int64_t n_f, const float* w_r, int64_t n_r, const int32_t* idx_f,
            int64_t ldif, const int32_t* idx_r, int64_t ldir, int64_t problems, double delta0,
            int32_t max_iterations, double rtol, double* out, int32_t* iters, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Multistate free energies (the MBAR equations behind `emus`, test.py:61-63,
 * and the driver of test.py:74-88), `problems` independent solves in one
 * launch.  u [rows, K] holds fp32 reduced energies, sample-major with row
 * stride ldu; problem p works on the N rows idx ? idx[p*ldi + n] : n (int32 row
 * gathers, e.g. stratified bootstrap resamples).  n_k (HOST int64[K], each >= 1,
 * summing to N) are the states' sample counts and f0 (HOST double[K], or null
 * for zeros) the start; both are read during the call and passed to the kernel
 * by value (the counts also as log n_k).  Inputs are promoted once; all
 * arithmetic is fp64 without contraction, in the gauge f_0 = 0.
 * One iteration at f: pass A accumulates, with a_k = (log n_k + f_k) - u_nk and
 * W_k = exp(a_k - max a) / sum_k exp(a_k - max a) in [0, 1], S_k = sum_n W_nk
 * and G_jk = sum_n W_nj W_nk; one lane forms f_sc = f - log(S / n), re-gauged,
 * and f_nr = f - H_r^{-1} g_r with g = S - n, H = diag(S) - G on states
 * 1..K-1 (Cholesky; a pivot not > 0 or a non-finite entry makes it invalid);
 * pass B evaluates |S - n|^2 at both, and f' = f_nr iff it is valid and its
 * norm is strictly smaller (a NaN falls to f_sc).  The loop stops when
 * max_i |f'_i - f_i| < rtol * max_i |f'_i| (from the first iteration on), at
 * max_iterations, or at once on a NaN iterate, which is returned; rtol = 0
 * returns exactly the max_iterations-th iterate.  f[p*K + k] = the last f',
 * iters[p] = iterations done, gram[p*K*K + j*K + k] = G_jk at the returned f
 * (the full symmetric matrix, from one more pass A).  Every loop exit compares
 * one LDS word read by all lanes: the trip count is workgroup-uniform and
 * bounded by max_iterations.
 * One workgroup per problem (256, 512 or 1024 threads by N * K alone, K >= 6
 * at most 512; grid-stride above 4096 problems), no atomics.  N * K <=
 * nfk_mbar_stage_cap(): the energies are gathered once into LDS, state-major;
 * otherwise every pass re-reads them through the index row.  Fixed-order
 * reductions: two runs are bitwise equal.  Index values are not validated.
 * NFK_EINVAL, nothing launched: !nfk_mbar_supported(K) (2 <= K <= 8), an
 * n_k < 1, sum n_k != N, problems < 1, max_iterations < 1, rtol < 0 or NaN,
 * ldu < K, ldi < N, null u / n_k / f / iters / gram, problems > 1 without idx.
 * ------------------------------------------------------------------------- */
int nfk_mbar_supported(int32_t K); /* host-only */
int nfk_mbar_stage_cap(void);      /* host-only: largest N * K kept in LDS */
int nfk_mbar(const float* u, int64_t ldu, int64_t N, int32_t K, const int64_t* n_k, const int32_t* idx,
             int64_t ldi, int64_t problems, const double* f0, int32_t max_iterations, double rtol,
             double* f, int32_t* iters, double* gram, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Metropolis chains over a batch of proposals (applications/src/utils.py:82-99),
 * nfk_metropolize.hip: `chains` independent chains of N steps in one launch.
 * Chain c reads e[c*lde + i] (reduced energies U/kT), lq[c*ldq + i] (log
 * proposal densities; lq null: the reference's energy-only rule) and
 * r[c*ldr + i] (uniforms in [0, 1)), all fp32.  Step i = 0 .. N-1 proposes
 * sample i, in fp32 without contraction and in this order:
 *   d = e_cur - e[i];  with lq: d = (d + lq_cur) - lq[i]
 *   accept iff r[i] < expf(d)       (nfk_hmc_accept's test; a NaN rejects)
 *   accepted: e_cur = e[i], lq_cur = lq[i], idx_cur = base + i
 * Start: carry_in == 0 -- the chain starts at proposal 0 (e_cur = e[0],
 * lq_cur = lq[0], idx_cur = base), so step 0 compares proposal 0 with itself,
 * as the reference's loop does; carry_in != 0 -- it starts from e_cur[c],
 * lq_cur[c] and idx_cur[c].  Whenever e_cur / lq_cur / idx_cur are given they
 * receive the final state, so a chain is continued batch by batch with
 * carry_in = 1 and `base` making the indices global.
 * Outputs, each nullable: state[c*lds + i] (int32) = idx_cur after step i;
 * accepted[c*lda + i] (uint8, 0 or 1); naccept[c] (int32) += the chain's
 * acceptances, as nfk_*_hmc_run adds; the carried state.
 * One wave per chain, four waves per workgroup, grid-stride over the chains.
 * A wave takes 64 consecutive proposals, one per lane; the pending lanes test
 * against the current state, a ballot finds the first that accepts, the state
 * moves to its values and the lanes after it stay pending, until the ballot is
 * empty: 1 + (acceptances in the block) rounds, each decision on the serial
 * loop's operands, hence the serial loop's bits.  No LDS, no atomics; ordinary
 * vector stores.  The arrays do not overlap.
 * NFK_EINVAL, nothing launched: chains or N below zero; base below zero or
 * base + N above INT32_MAX; and, with chains > 0 and N > 0, a null e or r;
 * exactly one of e_cur / idx_cur; lq_cur without e_cur, or with e_cur exactly
 * one of lq / lq_cur; carry_in without e_cur; with chains > 1 a row stride
 * (lde, ldr, ldq with lq, lds with state, lda with accepted) below N.
 * chains == 0 or N == 0 returns 0 without a launch.
 * ------------------------------------------------------------------------- */
int nfk_metropolize(const float* e, int64_t lde, const float* lq, int64_t ldq, const float* r, int64_t ldr,
                    int64_t chains, int64_t N, int32_t base, int32_t carry_in, float* e_cur, float* lq_cur,
                    int32_t* idx_cur, int32_t* state, int64_t lds, uint8_t* accepted, int64_t lda,
                    int32_t* naccept, nfk_stream_t stream);

/* ---------------------------------------------------------------------------
 * Weighted pair-distance histogram of a batch of configurations, the counts
 * behind the radial distribution function g(r) (nfk_pair_hist.hip; the
 * reference has no counterpart, its drivers stop at plot_Q).
 * x holds `batch` rows of n * dim fp32 (row stride ldx); w (nullable: 1 for every
 * row) one fp64 weight per row.  For every row b and every pair i < j, in fp32:
 *   d = x_i - x_j per component; with a box (lx, ly and, for dim 3, lz > 0)
 *   the minimum image d - L * rint(d * (1 / L)) per component, so positions
 *   need not lie in the box or within one box length of each other; with box
 *   lengths 0 no wrap (lz is ignored for dim 2);
 *   r = sqrt(sum d^2), k = (int)(r * (float)(nbins / r_max));
 *   the pair counts in bin k iff r < (float)r_max and k < nbins.
 * Pairs at or beyond r_max land in no bin, and so do pairs whose r is NaN or
 * infinite (the compare is false; there is no status word).
 *   hist[k] = sum_b w_b * count_b[k]      (fp64 [nbins])
 * A row's counts are uint32 in LDS (integer adds: any order); w_b multiplies
 * them in fp64 when the row is folded into its wave's accumulator.  Workgroup g
 * of nfk_pair_hist_parts(batch) takes, with its four waves v, the rows
 * (t * parts + g) * 4 + v, t = 0, 1, ..; it adds its accumulators in wave order
 * into partial g of `workspace` (fp64, nfk_pair_hist_workspace_elems(batch,
 * nbins) = parts * nbins elements, caller-owned), and a second launch on the
 * same stream adds the partials in index order into hist.  No floating-point
 * atomics and no host sync: capturable on one stream; for a given input and
 * batch, hist is bitwise the same run to run, and with unit weights every entry
 * is an exact integer while it stays below 2^53.
 * NFK_EINVAL, nothing launched: !nfk_pair_hist_supported(n, dim, nbins)
 * (1 <= n <= 256, dim 2 or 3, 1 <= nbins <= 1024); batch < 0; null hist; with
 * batch > 0 a null x or workspace; r_max not a number > 0; a negative or
 * non-finite box length, or some positive and some zero; a box with r_max >
 * min(L) / 2; ldx < n * dim with batch > 1.  batch == 0 writes zeros to hist.
 * ------------------------------------------------------------------------- */
int nfk_pair_hist_supported(int32_t n, int32_t dim, int32_t nbins); /* host-only */
int64_t nfk_pair_hist_parts(int64_t batch);                         /* host-only: partials, by batch alone */
int64_t nfk_pair_hist_workspace_elems(int64_t batch, int32_t nbins); /* host-only: fp64 elements */
int nfk_pair_hist(const float* x, int64_t ldx, const double* w, int64_t batch, int32_t n, int32_t dim,
                  double lx, double ly, double lz, double r_max, int32_t nbins, double* hist,
                  double* workspace, nfk_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NFK_H_ */
