"""ctypes binding of libnfk.so (include/nfk.h).

The product path has no CPU or eager-PyTorch fallback: if the HIP library is
missing or was built for a different ABI, every call raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NFK_LIBRARY", os.path.join(_HERE, "libnfk.so"))
ABI_VERSION = 4

NFK_EINVAL = -1
ST_INSIDE_SEEN = 1
ST_NEG_DISC = 2
ST_NAN_Z = 4

P = ctypes.c_void_p
I32 = ctypes.c_int32
I64 = ctypes.c_int64
F64 = ctypes.c_double
F32 = ctypes.c_float

# name -> (restype, argtypes); mirrors include/nfk.h one-to-one
SIGNATURES = {
    "nfk_abi_version": (ctypes.c_int, []),
    "nfk_last_error": (ctypes.c_char_p, []),
    "nfk_maf": (ctypes.c_int, [
        P, I64, P, P, I64,              # x, ldx, init_param, params, ldp
        I32, I32, I32, P, I64,          # c0, c1, dim, out, ldo
        P, I32, I64, I32, P]),          # logdet, logdet_mode, batch, inverse, stream
    "nfk_actnorm": (ctypes.c_int, [
        P, I64, P, P, I32, P, I64,      # x, ldx, mu, log_sigma, dim, z, ldz
        P, I32, P, I64, I32, P]),       # logdet, logdet_mode, ld_scalar, batch, inverse, stream
    "nfk_rqs_coupling_bwd": (ctypes.c_int, [
        P, I64, P,                      # x, ldx, params
        P, P, I32,                      # up_in, up_out, n_up
        P, P, I32,                      # lo_in, lo_out, n_lo
        P, I64, P,                      # gz, ldgz, glogdet
        P, P, I64, I64, I32,            # gparams, gx, ldgx, batch, K
        F64, F64, F64, F64, I32,        # left, right, bottom, top, tails
        F64, F64, F64,                  # min_bin_width, min_bin_height, min_derivative
        I32, I32, P]),                  # param_mode, inverse, stream
    "nfk_rqs_coupling": (ctypes.c_int, [
        P, I64, P,                      # x, ldx, params
        P, P, I32,                      # up_in, up_out, n_up
        P, P, I32,                      # lo_in, lo_out, n_lo
        P, I64, P, I32,                 # z, ldz, logdet, logdet_mode
        P, I64, I64, I32,               # lad_out, ld_lad, batch, K
        F64, F64, F64, F64, I32,        # left, right, bottom, top, tails
        F64, F64, F64,                  # min_bin_width, min_bin_height, min_derivative
        I32, I32, P, P]),               # param_mode, inverse, status, stream
    "nfk_searchsorted": (ctypes.c_int, [P, P, P, I64, I32, F64, P]),
    "nfk_affine_coupling": (ctypes.c_int, [P, I64, P, P, I64, P, I64, P, I32, I64, I32, I32, P]),
    "nfk_planar": (ctypes.c_int, [P, I64, P, P, P, P, I64, P, I32, P, I64, I32, I32, P]),
    "nfk_radial_workspace_elems": (ctypes.c_int64, []),
    "nfk_radial_sumsq": (ctypes.c_int, [P, I64, P, I64, I32, P, P, P]),
    "nfk_radial_apply": (ctypes.c_int, [P, I64, P, P, P, P, P, I64, P, P, I32, I64, I32, P]),
    "nfk_normal_logprob": (ctypes.c_int, [P, I64, P, P, I64, I32, F32, F32, I32, P, P]),
    "nfk_trig_features": (ctypes.c_int, [P, I64, P, I64, I64, I32, F64, P]),
    "nfk_fused_ar_supported": (ctypes.c_int, [I32, I32, I32]),
    "nfk_fused_ar_inverse_supported": (ctypes.c_int, [I32, I32, I32]),
    "nfk_fused_ar_pack_elems": (ctypes.c_int64, [I32, I32, I32]),
    "nfk_fused_ar_pack": (ctypes.c_int, [P, P, I32, I32, I32, P, P]),
    "nfk_fused_ar": (ctypes.c_int, [
        P, I64, P, I32, I32, I32,       # x, ldx, pack, dim, hidden, K
        F64, P, I64, P, I32,            # tail_bound, out, ldo, logdet, logdet_mode
        I64, I32, P, P]),               # batch, inverse, status, stream
    "nfk_gather_cols_ones": (ctypes.c_int, [P, I64, P, I32, I64, P, I64, P]),
    "nfk_fused_ar_workspace": (ctypes.c_int64, [I32, I32, I32, I64, I32]),
    "nfk_fused_ar_ws": (ctypes.c_int, [
        P, I64, P, I32, I32, I32,       # x, ldx, pack, dim, hidden, K
        F64, P, I64, P, I32,            # tail_bound, out, ldo, logdet, logdet_mode
        I64, I32, P, P, I64, P]),       # batch, inverse, status, workspace, workspace_floats, stream
    "nfk_fused_nsf_supported": (ctypes.c_int, [I32, I32, I32, I32]),
    "nfk_fused_nsf_pack_elems": (ctypes.c_int64, [I32, I32, I32, I32]),
    "nfk_fused_nsf_pack": (ctypes.c_int, [P, P, P, P, P, P, I32, I32, I32, I32, P, P]),
    "nfk_fused_nsf": (ctypes.c_int, [
        P, I64, P,                      # x, ldx, wpack
        P, P, I32,                      # up_in, up_out, n_up
        P, P, I32, I32,                 # lo_in, lo_out, n_lo, hidden
        P, I64, P, I32,                 # z, ldz, logdet, logdet_mode
        I64, I32, F64, I32, P, P]),     # batch, K, tail_bound, inverse, status, stream
    "nfk_fused_nsf_workspace": (ctypes.c_int64, [I32, I32, I32, I32, I64, I32]),
    "nfk_fused_nsf_ws": (ctypes.c_int, [
        P, I64, P, P, P, I32, P, P, I32, I32,   # x, ldx, wpack, up_in, up_out, n_up, lo_in, lo_out, n_lo, hidden
        P, I64, P, I32, I64, I32, F64, I32, P,  # z, ldz, logdet, mode, batch, K, tail_bound, inverse, status
        P, I64, P]),                            # workspace, workspace_floats, stream
    "nfk_fused_nsf_chain_max": (ctypes.c_int, [I32, I32, I32, I32]),
    "nfk_fused_nsf_chain": (ctypes.c_int, [
        P, I64, P, P, I32,              # x, ldx, wpacks, cmaps, nlayers
        I32, I32, I32,                  # n_lo, n_up, hidden
        P, I64, P, I32,                 # z, ldz, logdet, logdet_mode
        I64, I32, F64, I32, P,          # batch, K, tail_bound, inverse, status
        P, F32, F32, P]),               # log_prob, prior_scale, prior_half_log_det, stream
    "nfk_fused_nsf_chain_saved_ok": (ctypes.c_int, [I32, I32, I32, I32, I32]),
    "nfk_fused_nsf_chain_saved": (ctypes.c_int, [
        P, I64, P, P, I32,              # x, ldx, wpacks, cmaps, nlayers
        I32, I32, I32,                  # n_lo, n_up, hidden
        P, I64, P, I32,                 # z, ldz, logdet, logdet_mode
        I64, I32, F64, P,               # batch, K, tail_bound, status
        P, I64, I64, P, P]),            # saves, ld_saves, save_stride, smaps, stream
    "nfk_fused_nsf_vjp_pack_elems": (ctypes.c_int64, [I32, I32, I32, I32]),
    "nfk_fused_nsf_vjp_pack": (ctypes.c_int, [P, P, P, P, P, P, I32, I32, I32, I32, P, P]),
    "nfk_fused_nsf_vjp": (ctypes.c_int, [
        P, I64, P, P, P, I32,           # x, ldx, vpack, up_in, up_out, n_up
        P, P, I32, I32,                 # lo_in, lo_out, n_lo, hidden
        P, I64, P,                      # gz, ldgz, glogdet
        P, P, I64,                      # gparams, gx, ldgx
        P, P, I64,                      # h1, h2, ldh
        I64, I32, F64, I32, P]),        # batch, K, tail_bound, inverse, stream
    "nfk_fused_realnvp_supported": (ctypes.c_int, [I32, I32]),
    "nfk_fused_realnvp_pack_elems": (ctypes.c_int64, [I32, I32]),
    "nfk_fused_realnvp_pack": (ctypes.c_int, [P, I32, I32, P, P]),
    "nfk_fused_realnvp": (ctypes.c_int, [
        P, I64, P, I32, I32,            # x, ldx, wpack, half_dim, hidden
        P, I64, P, I32,                 # z, ldz, logdet, logdet_mode
        I64, I32, P]),                  # batch, inverse, stream
    "nfk_fcnn_dh_pack_floats": (ctypes.c_int64, [I32, I32]),
    "nfk_fcnn_dh_pack": (ctypes.c_int, [P, I32, I32, P, P]),
    "nfk_fcnn_dh": (ctypes.c_int, [P, I64, I32, P, P, I64, I32, P, I64, I64, I32, I64, P]),
    "nfk_fcnn_linear": (ctypes.c_int, [P, I64, I32, P, P, I32, I32, P, I64, I64, P]),
    "nfk_wlin_pack_floats": (ctypes.c_int64, [I32, I32]),
    "nfk_wlin_pack": (ctypes.c_int, [P, I32, I32, P, P]),
    "nfk_wide_rnvp_supported": (ctypes.c_int, [I32, I32]),
    "nfk_wide_rnvp_workspace": (ctypes.c_int64, [I32, I32, I64]),
    "nfk_wide_rnvp": (ctypes.c_int, [P, I64, P, P, I32, I32, P, I64, P, I32, I64, I32, P, I64, P]),
    "nfk_wide_rnvp_chain_workspace": (ctypes.c_int64, [I32, I32, I64]),
    "nfk_wide_rnvp_chain": (ctypes.c_int, [P, I64, P, P, I32, I32, I32, P, I64, P, I32, I64, I32, P, I64, P]),
    "nfk_ar_seqinv_supported": (ctypes.c_int, [I32, I32, I32]),
    "nfk_ar_seqinv_workspace": (ctypes.c_int64, [I32, I32, I32, I64]),
    "nfk_ar_seqinv": (ctypes.c_int, [P, I64, P, P, I32, I32, I32, ctypes.c_double, P, I64, P, I32, I64, P, P, I64,
                                     P]),
    "nfk_flows_bwd_workspace_bytes": (ctypes.c_int64, [I64, I32]),
    "nfk_planar_bwd": (ctypes.c_int, [
        P, I64, P, P, P,                # x, ldx, w, u, b
        P, I64, P, P, I64,              # gz, ldgz, glogdet, gx, ldgx
        P, P, P, P, I64, I32, I32, P]),  # gw, gu, gb, workspace, batch, dim, nonlinearity, stream
    "nfk_actnorm_bwd": (ctypes.c_int, [
        P, I64, P, P, I32,              # x, ldx, mu, log_sigma, dim
        P, I64, P, P, I64,              # gz, ldgz, gld_scalar, gx, ldgx
        P, P, P, I64, I32, P]),         # gmu, gls, workspace, batch, inverse, stream
    "nfk_radial_bwd_scalars": (ctypes.c_int, [
        P, I64, P, P, P, P,             # x, ldx, x0, log_alpha, beta, sumsq
        P, I64, P, P, P, I64, I32, P]),  # gz, ldgz, gld_scalar, scal, workspace, batch, dim, stream
    "nfk_radial_bwd_apply": (ctypes.c_int, [
        P, I64, P, P, I64, P,           # x, ldx, x0, gz, ldgz, scal
        P, I64, P, P, I64, I32, P]),    # gx, ldgx, gx0, workspace, batch, dim, stream
    "nfk_maf_bwd": (ctypes.c_int, [
        P, I64, P, P, I64,              # x, ldx, init_param, params, ldp
        P, I64, P, I32, I32, I32,       # gout, ldgo, glogdet, c0, c1, dim
        P, I64, P, I64, P, P,           # gx, ldgx, gparams, ldgp, ginit, workspace
        I64, I32, P]),                  # batch, inverse, stream
    "nfk_trig_features_bwd": (ctypes.c_int, [P, I64, P, I64, P, I64, I64, I32, F64, P]),
    "nfk_affine_coupling_bwd": (ctypes.c_int, [
        P, I64, P, P, I64,              # x_in, ld_in, s, t, ld_st
        P, I64, P,                      # g_out, ld_g, g_logdet
        P, I64, I32, P, P, I64,         # g_in, ld_gin, accumulate, g_s, g_t, ld_gst
        I64, I32, I32, P]),             # batch, n, inverse, stream
    "nfk_fused_realnvp_chain_max": (ctypes.c_int, [I32, I32]),
    "nfk_fused_realnvp_chain": (ctypes.c_int, [
        P, I64, P, I32,                 # x, ldx, wpacks, nlayers
        I32, I32,                       # half_dim, hidden
        P, I64, P, I32,                 # z, ldz, logdet, logdet_mode
        I64, I32, P,                    # batch, inverse, status
        P, F32, F32, P]),               # log_prob, prior_scale, prior_half_log_det, stream
    "nfk_einstein_logprob": (ctypes.c_int, [
        P, I64, P, P, P,                # z, ldz, centers, logdet, out
        I64, I32, I32, F32, F32,        # batch, natoms, dim, scale, half_log_det
        I32, F64, I32, P, P]),          # has_box, boxlength, sign, status, stream
    "nfk_einstein_logprob_bwd": (ctypes.c_int, [
        P, I64, P, P, P, I64,           # z, ldz, centers, g, gz, ldgz
        I64, I32, I32, F32,             # batch, natoms, dim, scale
        I32, F64, P]),                  # has_box, boxlength, stream
    "nfk_gmix_supported": (ctypes.c_int, [I32, I32]),
    "nfk_gmix_logprob": (ctypes.c_int, [
        P, I64, P, P, P, P, P,          # x, ldx, centers, scales, hlds, logdet, out
        I64, I32, I32, I32,             # batch, npart, dim, ncenters
        I32, P, P]),                    # sign, status, stream
    "nfk_gmix_logprob_bwd": (ctypes.c_int, [
        P, I64, P, P, P, P, P, I64,     # x, ldx, centers, scales, hlds, g, gx, ldgx
        I64, I32, I32, I32, P]),        # batch, npart, dim, ncenters, stream
    "nfk_lj_supported": (ctypes.c_int, [I32, I32]),
    "nfk_lj_potential": (ctypes.c_int, [
        P, I64, P, I64, I32, I32,       # x, ldx, out, batch, n, dim
        F64, F64, F64, I32, F64, I32, P]),  # boxlength, sigma, epsilon, has_cutoff, cutoff, shift, stream
    "nfk_lj_potential_bwd": (ctypes.c_int, [
        P, I64, P, P, I64,              # x, ldx, g, gx, ldgx
        I64, I32, I32,                  # batch, n, dim
        F64, F64, F64, I32, F64, I32, P]),  # boxlength, sigma, epsilon, has_cutoff, cutoff, shift, stream
    "nfk_eam_supported": (ctypes.c_int, [I32]),
    "nfk_eam_potential": (ctypes.c_int, [
        P, I64, P, I64, I32,            # x, ldx, out, batch, n
        P, I32, F64, P, I32, F64,       # rtab, nr, dr, ftab, nrho, drho
        F64, F64, F64, F64, F64, F64, P]),  # f_end, fp_end, lx, ly, lz, rc, stream
    "nfk_eam_potential_bwd": (ctypes.c_int, [
        P, I64, P, P, I64,              # x, ldx, g, gx, ldgx
        I64, I32,                       # batch, n
        P, I32, F64, P, I32, F64,       # rtab, nr, dr, ftab, nrho, drho
        F64, F64, F64, F64, F64, F64, P]),  # f_end, fp_end, lx, ly, lz, rc, stream
    "nfk_einstein_trajectory": (ctypes.c_int, [
        P, I64, P, I64, P, I64, P, I64, P,  # x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out
        I64, I32, F64, F64, I32,        # batch, path_len, dt, dt_sq, scheme
        P, I32, I32, F32, F32,          # centers, natoms, dim, scale, half_log_det
        I32, F64, P]),                  # has_box, boxlength, stream
    "nfk_gmix_trajectory": (ctypes.c_int, [
        P, I64, P, I64, P, I64, P, I64, P,  # x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out
        I64, I32, F64, F64, I32,        # batch, path_len, dt, dt_sq, scheme
        P, P, P, I32, I32, I32, P]),    # centers, scales, hlds, npart, dim, ncenters, stream
    "nfk_lj_trajectory": (ctypes.c_int, [
        P, I64, P, I64, P, I64, P, I64, P,  # x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out
        I64, I32, F64, F64, I32,        # batch, path_len, dt, dt_sq, scheme
        I32, I32,                       # n, dim
        F64, F64, F64, I32, F64, I32, P]),  # boxlength, sigma, epsilon, has_cutoff, cutoff, shift, stream
    "nfk_eam_trajectory": (ctypes.c_int, [
        P, I64, P, I64, P, I64, P, I64, P,  # x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out
        I64, I32, F64, F64, I32,        # batch, path_len, dt, dt_sq, scheme
        I32,                            # n
        P, I32, F64, P, I32, F64,       # rtab, nr, dr, ftab, nrho, drho
        F64, F64, F64, F64, F64, F64, P]),  # f_end, fp_end, lx, ly, lz, rc, stream
    "nfk_hmc_accept": (ctypes.c_int, [
        P, I64, P, I64, P, P,           # x_cur, ldc, x_new, ldn, u_cur, u_new
        P, P, P, P,                     # k_cur, k_new, r, naccept
        I64, I32, F64, P]),             # chains, width, beta, stream
    "nfk_einstein_hmc_supported": (ctypes.c_int, [I32, I32]),
    "nfk_gmix_hmc_supported": (ctypes.c_int, [I32, I32, I32]),
    "nfk_lj_hmc_supported": (ctypes.c_int, [I32, I32]),
    "nfk_einstein_hmc_run": (ctypes.c_int, [
        P, I64, P, P, P, P, P, I64, P, P,   # x_cur, ldx, u_cur, naccept, v_draws, r, v_last, ldv, pos_rec, pot_rec
        I64, I32, I32, F64, F64, I32,   # chains, epochs, path_len, dt, dt_sq, scheme
        F64, I32,                       # beta, hamiltonian
        P, I32, I32, F32, F32,          # centers, natoms, dim, scale, half_log_det
        I32, F64, P]),                  # has_box, boxlength, stream
    "nfk_gmix_hmc_run": (ctypes.c_int, [
        P, I64, P, P, P, P, P, I64, P, P,   # x_cur, ldx, u_cur, naccept, v_draws, r, v_last, ldv, pos_rec, pot_rec
        I64, I32, I32, F64, F64, I32,   # chains, epochs, path_len, dt, dt_sq, scheme
        F64, I32,                       # beta, hamiltonian
        P, P, P, I32, I32, I32, P]),    # centers, scales, hlds, npart, dim, ncenters, stream
    "nfk_lj_hmc_run": (ctypes.c_int, [
        P, I64, P, P, P, P, P, I64, P, P,   # x_cur, ldx, u_cur, naccept, v_draws, r, v_last, ldv, pos_rec, pot_rec
        I64, I32, I32, F64, F64, I32,   # chains, epochs, path_len, dt, dt_sq, scheme
        F64, I32,                       # beta, hamiltonian
        I32, I32,                       # n, dim
        F64, F64, F64, I32, F64, I32, P]),  # boxlength, sigma, epsilon, has_cutoff, cutoff, shift, stream
    "nfk_eam_hmc_supported": (ctypes.c_int, [I32]),
    "nfk_eam_hmc_run": (ctypes.c_int, [
        P, I64, P, P, P, P, P, I64, P, P,   # x_cur, ldx, u_cur, naccept, v_draws, r, v_last, ldv, pos_rec, pot_rec
        I64, I32, I32, F64, F64, I32,   # chains, epochs, path_len, dt, dt_sq, scheme
        F64, I32,                       # beta, hamiltonian
        I32,                            # n
        P, I32, F64, P, I32, F64,       # rtab, nr, dr, ftab, nrho, drho
        F64, F64, F64, F64, F64, F64, P]),  # f_end, fp_end, lx, ly, lz, rc, stream
    "nfk_philox_fill": (ctypes.c_int, [
        P, I32, I64, I32, I32,          # out, normals, rows, n, dim
        I64, I64, I64, I32, I32, P]),   # step, row_base, seed, tag, zero_mean, stream
    "nfk_einstein_langevin": (ctypes.c_int, [
        P, I64, P, I64, P, I64, P, I64, P,  # x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out
        I64, I32, I64, I64, I64, I32,   # batch, nsteps, step0, row_base, seed, zero_mean
        F32, F32, F32, F32, I32, P, P,  # hb, hd, c1, c2, record_every, pos_rec, pot_rec
        P, I32, I32, F32, F32,          # centers, natoms, dim, scale, half_log_det
        I32, F64, P]),                  # has_box, boxlength, stream
    "nfk_gmix_langevin": (ctypes.c_int, [
        P, I64, P, I64, P, I64, P, I64, P,  # x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out
        I64, I32, I64, I64, I64, I32,   # batch, nsteps, step0, row_base, seed, zero_mean
        F32, F32, F32, F32, I32, P, P,  # hb, hd, c1, c2, record_every, pos_rec, pot_rec
        P, P, P, I32, I32, I32, P]),    # centers, scales, hlds, npart, dim, ncenters, stream
    "nfk_lj_langevin": (ctypes.c_int, [
        P, I64, P, I64, P, I64, P, I64, P,  # x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out
        I64, I32, I64, I64, I64, I32,   # batch, nsteps, step0, row_base, seed, zero_mean
        F32, F32, F32, F32, I32, P, P,  # hb, hd, c1, c2, record_every, pos_rec, pot_rec
        I32, I32,                       # n, dim
        F64, F64, F64, I32, F64, I32, P]),  # boxlength, sigma, epsilon, has_cutoff, cutoff, shift, stream
    "nfk_eam_langevin": (ctypes.c_int, [
        P, I64, P, I64, P, I64, P, I64, P,  # x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, pot_out
        I64, I32, I64, I64, I64, I32,   # batch, nsteps, step0, row_base, seed, zero_mean
        F32, F32, F32, F32, I32, P, P,  # hb, hd, c1, c2, record_every, pos_rec, pot_rec
        I32,                            # n
        P, I32, F64, P, I32, F64,       # rtab, nr, dr, ftab, nrho, drho
        F64, F64, F64, F64, F64, F64, P]),  # f_end, fp_end, lx, ly, lz, rc, stream
    "nfk_lj_switch": (ctypes.c_int, [
        P, I64, P, I64, P, I64, P, I64, P,  # x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, en_out
        I64, I32, I64, I64, I64, I32,   # batch, nsteps, step0, row_base, seed, zero_mean
        F32, F32, F32, F32, I32, P, P,  # hb, hd, c1, c2, record_every, pos_rec, en_rec
        I32, I32,                       # n, dim
        F64, F64, F64, I32, F64, I32,   # boxlength, sigma, epsilon, has_cutoff, cutoff, shift
        P, I32, I32, F32, F32, I32, F64,  # centers, natoms_A, dim_A, scale, half_log_det, has_box, boxlength_A
        P, I64, F64, F32, P, P]),       # lam, lam_len, inv_kT, kT, work, stream
    "nfk_eam_switch": (ctypes.c_int, [
        P, I64, P, I64, P, I64, P, I64, P,  # x_in, ldxi, v_in, ldvi, x_out, ldxo, v_out, ldvo, en_out
        I64, I32, I64, I64, I64, I32,   # batch, nsteps, step0, row_base, seed, zero_mean
        F32, F32, F32, F32, I32, P, P,  # hb, hd, c1, c2, record_every, pos_rec, en_rec
        I32,                            # n
        P, I32, F64, P, I32, F64,       # rtab, nr, dr, ftab, nrho, drho
        F64, F64, F64, F64, F64, F64,   # f_end, fp_end, lx, ly, lz, rc
        P, I32, I32, F32, F32, I32, F64,  # centers, natoms_A, dim_A, scale, half_log_det, has_box, boxlength_A
        P, I64, F64, F32, P, P]),       # lam, lam_len, inv_kT, kT, work, stream
    "nfk_bar_stage_cap": (ctypes.c_int, []),
    "nfk_bar": (ctypes.c_int, [
        P, I64, P, I64,                 # w_f, n_f, w_r, n_r
        P, I64, P, I64,                 # idx_f, ldif, idx_r, ldir
        I64, F64, I32, F64,             # problems, delta0, max_iterations, rtol
        P, P, P]),                      # out, iters, stream
    "nfk_mbar_supported": (ctypes.c_int, [I32]),
    "nfk_mbar_stage_cap": (ctypes.c_int, []),
    "nfk_mbar": (ctypes.c_int, [
        P, I64, I64, I32, P,            # u, ldu, N, K, n_k (host int64[K])
        P, I64, I64, P,                 # idx, ldi, problems, f0 (host double[K] or null)
        I32, F64,                       # max_iterations, rtol
        P, P, P, P]),                   # f, iters, gram, stream
    "nfk_metropolize": (ctypes.c_int, [
        P, I64, P, I64, P, I64,         # e, lde, lq, ldq, r, ldr
        I64, I64, I32, I32,             # chains, N, base, carry_in
        P, P, P,                        # e_cur, lq_cur, idx_cur
        P, I64, P, I64, P, P]),         # state, lds, accepted, lda, naccept, stream
    "nfk_pair_hist_supported": (ctypes.c_int, [I32, I32, I32]),
    "nfk_pair_hist_parts": (ctypes.c_int64, [I64]),
    "nfk_pair_hist_workspace_elems": (ctypes.c_int64, [I64, I32]),
    "nfk_pair_hist": (ctypes.c_int, [
        P, I64, P, I64, I32, I32,       # x, ldx, w, batch, n, dim
        F64, F64, F64, F64, I32,        # lx, ly, lz, r_max, nbins
        P, P, P]),                      # hist, workspace, stream
}

_lock = threading.Lock()
_lib = None


class NfkError(RuntimeError):
    """A libnfk.so entry point returned an error code."""


def load():
    """Load (once) and return the library; raise if it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "normalizingflow_amd: HIP kernel library not found at %s -- build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
                "normalizingflow_amd/csrc`); there is no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        ver = lib.nfk_abi_version()
        if ver != ABI_VERSION:
            raise ImportError("libnfk.so ABI %d != expected %d; rebuild" % (ver, ABI_VERSION))
        _lib = lib
    return _lib


def call(name, *args):
    """Invoke an entry point and turn a non-zero return into an exception."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        msg = load().nfk_last_error()
        msg = msg.decode() if msg else ""
        if rc == NFK_EINVAL:
            raise ValueError("%s: %s" % (name, msg))
        raise NfkError("%s failed (hipError %d): %s" % (name, rc, msg))
    return rc
