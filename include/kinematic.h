#pragma once
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
void kinematic_err_fun(double *nom_x, double *delta_x, double *out);
void kinematic_inv_err_fun(double *nom_x, double *true_x, double *out);
void kinematic_H_mod_fun(double *state, double *out);
void kinematic_f_fun(double *state, double dt, double *out);
void kinematic_F_fun(double *state, double dt, double *out);
void kinematic_h_1(double *state, double *unused1, double *out);
void kinematic_H_1(double *state, double *unused1, double *out);
void kinematic_dims(int *dims);
int kinematic_kind_zdim(int kind);
int kinematic_kind_maha(int kind);
int kinematic_num_kinds(void);
void kinematic_kinds(int *out);
int kinematic_last_error(void);
const char *kinematic_last_error_string(void);
void kinematic_clear_error(void);
int kinematic_batch_predict(double *x, double *P, const double *Q, const double *dt_vec, double dt, int64_t n, int norm_quats, void *stream);
int kinematic_batch_update_1(double *x, double *P, double *z, const double *R, int r_per_filter, const double *ea, int64_t n, int norm_quats, uint8_t *flags, void *stream);
int kinematic_batch_predict_update_1(double *x, double *P, const double *Q, const double *dt_vec, double dt, double *z, const double *R, int r_per_filter, const double *ea, int64_t n, int norm_quats, uint8_t *flags, void *stream);
int kinematic_batch_predict_masked(double *x, double *P, const double *Q, const double *dt_vec, double dt, int64_t n, int norm_quats, const uint8_t *active, void *stream);
int kinematic_batch_update_1_masked(double *x, double *P, double *z, const double *R, int r_per_filter, const double *ea, int64_t n, int norm_quats, uint8_t *flags, const uint8_t *active, void *stream);
int kinematic_batch_predict_update_1_masked(double *x, double *P, const double *Q, const double *dt_vec, double dt, double *z, const double *R, int r_per_filter, const double *ea, int64_t n, int norm_quats, uint8_t *flags, const uint8_t *active, void *stream);
int kinematic_batch_predict_update_1_ckpt(double *x, double *P, const double *Q, const double *dt_vec, double dt, double *z, const double *R, int r_per_filter, const double *ea, int64_t n, int norm_quats, uint8_t *flags, double *ckpt_x, double *ckpt_P, double *ckpt_z, void *stream);
int kinematic_batch_ring_copy(double *ring, int64_t ring_stride, double *flat, int64_t flat_stride, int64_t rec, const int32_t *slot, const uint8_t *active, int64_t n, int to_ring, void *stream);
int kinematic_batch_flags_set(uint8_t *flags, const uint8_t *mask, int value, int64_t n, void *stream);
int kinematic_batch_timeline_plan(const double *t, const uint8_t *active, const double *ft, int64_t n, double *dt_out, uint8_t *act_out, uint8_t *late_out, int32_t *n_late, const double *z_src, double *z_keep, int64_t z_count, void *stream);
int kinematic_batch_timeline_push(const double *t, const uint8_t *act, double *ft, const double *x, const double *P, int64_t n, int64_t K, int64_t nmax, double *ring_t, double *ring_x, double *ring_P, int32_t *ring_kind, int32_t *ring_nobs, double *ring_z, double *ring_R, double *ring_ea, int64_t *ring_head, int64_t *ring_length, int kind, int nobs, const double *z_obs, int64_t z_stride_f, int64_t z_stride_o, const double *R, int r_per_filter, int64_t r_stride_f, int64_t r_stride_o, const double *ea, int64_t ea_stride_f, int64_t ea_stride_o, void *stream);
int kinematic_has_step_kinds(void);
int kinematic_batch_predict_update_kinds(double *x, double *P, const double *Q, const double *dt_vec, double dt, const int32_t *kinds, double *z, const double *R, int r_per_filter, int64_t n, int norm_quats, uint8_t *flags, const uint8_t *active, void *stream);
int kinematic_batch_update_kinds(double *x, double *P, const int32_t *kinds, double *z, const double *R, int r_per_filter, int64_t n, int norm_quats, uint8_t *flags, const uint8_t *active, void *stream);
int kinematic_batch_timeline_push_kinds(const double *t, const uint8_t *act, double *ft, const double *x, const double *P, int64_t n, int64_t K, int64_t nmax, double *ring_t, double *ring_x, double *ring_P, int32_t *ring_kind, int32_t *ring_nobs, double *ring_z, double *ring_R, double *ring_ea, int64_t *ring_head, int64_t *ring_length, const int32_t *kinds, const double *z_obs, const double *R, int r_per_filter, void *stream);
int kinematic_batch_rewind_locate(const uint8_t *late, const double *t, int64_t n, int64_t K, double *ring_t, double *ring_x, double *ring_P, int64_t *ring_head, int64_t *ring_length, double max_rewind_age, double *x, double *P, double *ft, double *dt_out, uint8_t *act_out, int32_t *rep_slot, int32_t *rep_n, uint8_t *drop_out, int32_t *counts, void *stream);
int kinematic_batch_rewind_fetch(const int32_t *rep_slot, const int32_t *rep_n, int64_t q, const double *t_prev, int64_t n, int64_t K, int64_t nmax, double *ring_t, int32_t *ring_kind, double *ring_z, double *ring_R, double *t_out, double *dt_out, int32_t *kinds_out, uint8_t *act_out, double *z_out, double *z_keep, double *R_out, void *stream);
int kinematic_batch_maha_1(const double *x, const double *P, const double *z, const double *R, int r_per_filter, const double *ea, int64_t n, double *d2, void *stream);
void kinematic_msckf_dims(int *dims);
int kinematic_kind_eadim(int kind);
int kinematic_zmax(void);
int kinematic_run_unroll(void);
int kinematic_has_batch_run(void);
int kinematic_predict_identity_at_dt0(void);
int kinematic_batch_run(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts, int64_t T, double *z, const double *R, int64_t n, int norm_quats, uint8_t *flags, double *trace_x, double *trace_P, const double *ea, const int32_t *augment, void *stream);
int kinematic_has_batch_run_pf(void);
int kinematic_batch_run_pf(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts, int64_t T, double *z, const double *R, int64_t n, int norm_quats, uint8_t *flags, double *trace_x, double *trace_P, void *stream);
int kinematic_has_batch_run_pf_r(void);
int kinematic_batch_run_pf_r(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts, int64_t T, double *z, const double *R, int64_t n, int norm_quats, uint8_t *flags, double *trace_x, double *trace_P, void *stream);
int kinematic_has_batch_run_pf_rd(void);
int kinematic_batch_run_pf_rd(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts, int64_t T, double *z, const double *R, int64_t n, int norm_quats, uint8_t *flags, double *trace_x, double *trace_P, void *stream);
int kinematic_has_batch_run_pf_ea(void);
int kinematic_batch_run_pf_ea(double *x, double *P, const double *Q, const int32_t *kinds, const double *dts, int64_t T, double *z, const double *R, int64_t n, int norm_quats, uint8_t *flags, double *trace_x, double *trace_P, const double *ea, const int32_t *augment, void *stream);
int kinematic_has_tri_trace(void);
int kinematic_batch_rts(const double *xf, const double *Pf, const double *ts, int64_t T, const double *Q, int64_t n, int norm_quats, double *xs, double *Ps, const double *x_last, const double *P_last, void *stream);
int kinematic_has_batch_rts_pf(void);
int kinematic_batch_rts_pf(const double *xf, const double *Pf, const double *dts, const uint8_t *act, int64_t T, const double *Q, int64_t n, int norm_quats, double *xs, double *Ps, const double *x_last, const double *P_last, void *stream);
void kinematic_predict(double *in_x, double *in_P, double *in_Q, double dt);
void kinematic_update_1(double *in_x, double *in_P, double *in_z, double *in_R, double *in_ea);
#ifdef __cplusplus
}
#endif
