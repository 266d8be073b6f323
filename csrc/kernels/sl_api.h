// The C ABI of libslkernels.so: every exported sl_* entry point, declared exactly once.
//
// This is the only place a signature is written besides its definition.  Every .hip file sees
// it through common.h, so a definition that disagrees with its declaration here stops the
// build ("conflicting types for ..."); serverless_learn_amd/ops/_native.py parses this file at
// import to derive the ctypes argtypes / restypes, and serverless_learn_amd/build.py refuses a
// library whose exported sl_* symbols are not exactly the names declared here.
//
// Because Python reads it, keep to what its small parser understands: one `RET NAME(PARAMS);`
// per entry point inside the extern "C" block; parameter types int, unsigned, long, long long,
// unsigned long long, float, double, any pointer, hipStream_t; return types int, long, void, or
// a pointer / hipStream_t for helpers only other .hip files call.  No macros in parameter
// lists, no default arguments, no function pointers.  What each argument means is documented on
// the definition.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace sl {
struct BnBwdEpi;  // bn_bwd_epi.h
}

extern "C" {

// cnn_aux.hip
long sl_rsum_floats(int n);
long sl_rsum_result_offset(int n);
int sl_deterministic();
int sl_input_norm(const uint8_t* x, const uint8_t* lab, const int* cursor, int n_batches, int batch, long img_pixels,
                  uint16_t* y, uint8_t* lab_out, float m0, float m1, float m2, float s0, float s1, float s2,
                  hipStream_t stream);
int sl_input_aug(const uint8_t* x, const uint8_t* lab, const int* cursor, int n_records, int batch, int H, int W,
                 int pad, int flags, unsigned long long seed, uint16_t* y, uint8_t* lab_out, int* params_out,
                 float m0, float m1, float m2, float s0, float s1, float s2, hipStream_t stream);
int sl_input_mix(const uint8_t* x, const uint8_t* lab, const int* cursor, int n_records, int batch, int H, int W,
                 int pad, int flags, unsigned long long seed, const int* table, int modes, uint16_t* y,
                 uint8_t* lab_out, int* params_out, int* mix_out, float m0, float m1, float m2, float s0, float s1,
                 float s2, hipStream_t stream);
int sl_cursor_bump(int* cursor, hipStream_t stream);
int sl_bn_finalize(const float* stats, const float* gamma, const float* beta, float* coef, float* run_mean,
                   float* run_var, int C, float count, float eps, float momentum, hipStream_t stream);
int sl_bn_apply(const uint16_t* x, const float* coef, const uint16_t* res, const float* rcoef, uint16_t* y, long rows,
                int C, int relu, int mode, hipStream_t stream);
int sl_bn_bwd_reduce(const uint16_t* dy, const uint16_t* y, const uint16_t* x, const float* mcoef,
                     const uint8_t* ymask, uint16_t* dz_out, float* sums, const uint16_t* x2, float* sums2, long rows,
                     int C, hipStream_t stream);
int sl_bn_bwd_finalize(const float* sums, const float* coef, float* dcoef, float* grad_gamma, float* grad_beta, int C,
                       float count, hipStream_t stream);
int sl_bn_bwd_apply(const uint16_t* dy, const uint16_t* y, const uint16_t* x, const float* dcoef, uint16_t* dx,
                    long rows, int C, hipStream_t stream);
int sl_bn_apply_stats(const uint16_t* x, const float* stats, const float* gamma, const float* beta, float* coef,
                      float* run_mean, float* run_var, const uint16_t* res, const float* rstats, const float* rgamma,
                      const float* rbeta, float* rcoef, float* rrun_mean, float* rrun_var, uint16_t* y,
                      uint8_t* mask_out, long rows, int C, int relu, int mode, float count, float eps, float momentum,
                      hipStream_t stream);
int sl_bn_bwd_apply_dual(const uint16_t* dz, const uint16_t* xa, const float* sums_a, const float* coef_a,
                         float* gg_a, float* gb_a, uint16_t* dx_a, const uint16_t* xb, const float* sums_b,
                         const float* coef_b, float* gg_b, float* gb_b, uint16_t* dx_b, long rows, int C, float count,
                         hipStream_t stream);
int sl_bn_bwd_apply_sums(const uint16_t* dy, const uint16_t* y, const uint16_t* x, const float* mcoef,
                         const float* sums, const float* coef, float* grad_gamma, float* grad_beta, uint16_t* dx,
                         long rows, int C, float count, hipStream_t stream);
int sl_maxpool_fwd(const uint16_t* x, uint16_t* y, uint8_t* arg, int N, int H, int W, int C, int OH, int OW, int K,
                   int s, int p, hipStream_t stream);
int sl_maxpool_bwd(const uint16_t* dy, const uint8_t* arg, uint16_t* dx, int N, int H, int W, int C, int OH, int OW,
                   int K, int s, int p, hipStream_t stream);
int sl_avgpool_fwd(const uint16_t* x, uint16_t* y, int N, int HW, int C, hipStream_t stream);
int sl_avgpool_bwd(const uint16_t* dy, uint16_t* dx, int N, int HW, int C, hipStream_t stream);
int sl_softmax_ce(const float* z, const uint8_t* lab, float* loss, float* correct, uint16_t* dz, int ldd,
                  float* dbias, int N, int ncls, float grad_scale, hipStream_t stream);
int sl_softmax_ce_soft(const float* z, const uint8_t* lab, float* loss, float* correct, uint16_t* dz, int ldd,
                       float* dbias, int N, int ncls, float grad_scale, const int* mix, float eps,
                       hipStream_t stream);
long sl_softmax_ce_wide_ws_floats(int N, int ldd);
int sl_softmax_ce_wide(const float* z, const uint8_t* lab, float* loss, float* correct, uint16_t* dz, int ldd,
                       float* dbias, int N, int ncls, float grad_scale, const int* mix, float eps, int soft,
                       float* ws, long ws_floats, hipStream_t stream);

// conv.hip (the sl_wgrad_* helpers and sl_conv_dgrad_bn are called from other .hip files, not from Python)
void sl_conv_note_kernel(int family);
int sl_conv_kernels_seen(int clear);
int sl_rsum_fold2(float* buf, float* buf2, int n, hipStream_t stream);
int sl_rsum_fold(float* buf, int n, hipStream_t stream);
int sl_conv_set_s2(int on);
int sl_conv_set_phase(int on);
int sl_conv_fwd(const uint16_t* x, int N, int H, int W, int C, const uint16_t* w, int cout, int KH, int KW,
                int stride, int pad, int OH, int OW, uint16_t* y, int ldy, float* yf, const float* bias, float* stats,
                hipStream_t stream);
int sl_conv_dgrad_bn(const uint16_t* dy, int N, int OH, int OW, int ldd, const uint16_t* wt, int cin, int KH, int KW,
                     int stride, int pad, int H, int W, uint16_t* dx, const uint16_t* add, const sl::BnBwdEpi* bn,
                     hipStream_t stream, int add_even);
int sl_conv_dgrad(const uint16_t* dy, int N, int OH, int OW, int ldd, const uint16_t* wt, int cin, int KH, int KW,
                  int stride, int pad, int H, int W, uint16_t* dx, const uint16_t* add, hipStream_t stream);
int sl_conv_dgrad_s2_even(const uint16_t* dy, int N, int OH, int OW, int ldd, const uint16_t* wt, int cin, int H,
                          int W, uint16_t* dx, hipStream_t stream);
int sl_conv_dgrad_bnx(const uint16_t* dy, int N, int OH, int OW, int ldd, const uint16_t* wt, int cin, int KH, int KW,
                      int stride, int pad, int H, int W, uint16_t* dx, const uint16_t* add, const uint16_t* bx,
                      const uint8_t* ymask, const float* mcoef, float* sums, const uint16_t* x2, float* sums2,
                      int add_even, hipStream_t stream);
long sl_conv_wgrad_ws_need();
void sl_wgrad_note_need(long floats);
int sl_wgrad_side_begin(hipStream_t side);
int sl_wgrad_side_join(hipStream_t main, int end);
void sl_wgrad_slab_acquire(const float* ws, hipStream_t main);
hipStream_t sl_wgrad_reduce_stream(hipStream_t main);
void sl_wgrad_reduce_done(const float* ws, hipStream_t rs);
int sl_wgrad_slab_reduce(const float* ws, int slices, long n, float* dw, hipStream_t stream);
int sl_conv_wgrad(const uint16_t* x, int N, int H, int W, int C, const uint16_t* dy, int ldy, int cout, int KH,
                  int KW, int stride, int pad, int OH, int OW, float* dw, int target_wgs, float* ws, long ws_floats,
                  hipStream_t stream);
int sl_conv_wt(const void* descs, int nd, long total, hipStream_t stream);
int sl_conv_wt_desc_size();

// conv3x3_halo.hip: direct kernels for 3x3/s1/p1 64->64 convolutions on 32-wide images
int sl_conv_set_halo(int on);
int sl_conv3x3_c64_applicable(int H, int W, int C, int cout, int KH, int KW, int stride, int pad, int ldw);
int sl_conv3x3_c64_bn(const uint16_t* src, const uint16_t* w, int cin, int flip, int N, int H, uint16_t* y, int ldy,
                      const uint16_t* add, float* stats, const sl::BnBwdEpi* bn, hipStream_t stream);
int sl_conv3x3_c64(const uint16_t* src, const uint16_t* w, int cin, int flip, int N, int H, uint16_t* y, int ldy,
                   const uint16_t* add, float* stats, hipStream_t stream);
int sl_conv3x3_bnin_fwd(const uint16_t* x, const uint16_t* w, int N, int H, uint16_t* y, int ldy, float* stats,
                        const float* bstats, const float* gamma, const float* beta, float* coef, float* run_mean,
                        float* run_var, float count, float eps, float momentum, hipStream_t stream);
int sl_conv3x3_wgrad_c64_applicable(int H, int W, int C, int cout, int KH, int KW, int stride, int pad, int ldy);
int sl_conv3x3_wgrad_c64(const uint16_t* x, const uint16_t* dy, int ldy, int N, int H, float* dw, float* ws,
                         long ws_floats, hipStream_t stream);
int sl_conv3x3_bnin_wgrad(const uint16_t* x, const uint16_t* dy, int N, int H, float* dw, float* ws, long ws_floats,
                          const float* bstats, const float* gamma, const float* beta, float count, float eps,
                          hipStream_t stream);

// datagen.hip
int sl_synth_images(uint8_t* img, uint8_t* lab, long n, int pixels, const float* protos, int classes, float noise,
                    float scale, float offset, unsigned long long seed, long first, hipStream_t stream);

// diag.hip
int sl_clock_probe(unsigned long long* buf, unsigned* cnt, int cap, hipStream_t stream);
int sl_comm_proxy(float* a, const float* b, long n, int nwg, hipStream_t stream);

// elementwise.hip
int sl_gossip_apply(float* m, float* o, const double* din, long kin, double alpha, double* dout, long n,
                    hipStream_t stream);
int sl_gossip_absorb(float* m, float* o, const double* r, long kr, double alpha, const double* sent, long ks, long n,
                     hipStream_t stream);
int sl_sgd_flat(float* w, const float* g, float* mom, uint16_t* shadow, long n, float lr, float mu, float wd,
                float gscale, hipStream_t stream);
int sl_adamw_flat(float* w, const float* g, float* mom, float* v, uint16_t* shadow, long n, const int* step,
                  const float* lr_tab, int lr_n, float lr, float wd, float gscale, float b1, float b2, float omb1,
                  float omb2, float lnb1, float lnb2, float eps, hipStream_t stream);
int sl_sgd_flat_lr(float* w, const float* g, float* mom, uint16_t* shadow, long n, const int* step,
                   const float* lr_tab, int lr_n, float mu, float wd, float gscale, hipStream_t stream);
int sl_adamw_flat_groups(float* w, const float* g, float* mom, float* v, uint16_t* shadow, long n, const int* step,
                         const float* lr_tab, int lr_n, float lr, float wd, float gscale, float b1, float b2,
                         float omb1, float omb2, float lnb1, float lnb2, float eps, const uint8_t* cls, float wd_norm,
                         float wd_bias, hipStream_t stream);
int sl_sgd_flat_lr_groups(float* w, const float* g, float* mom, uint16_t* shadow, long n, const int* step,
                          const float* lr_tab, int lr_n, float lr, float mu, float wd, float gscale,
                          const uint8_t* cls, float wd_norm, float wd_bias, hipStream_t stream);
int sl_clip_grad_partials(long n);
int sl_clip_grad_norm(float* g, long n, float max_norm, double* partials, int n_partials, float* norm_out,
                      hipStream_t stream);
int sl_accum_flat(float* dst, const float* src, long n, int add, hipStream_t stream);
int sl_ema_flat(float* ema, const float* w, long n, int* step, unsigned* ticket, const float* omd_tab, int tab_n,
                hipStream_t stream);
int sl_to_bf16(const float* src, uint16_t* dst, long n, hipStream_t stream);

// eval_metrics.hip
int sl_eval_accum_wide(const float* logits, int ld, const uint8_t* lab, const float* loss_rows, int rows, int n_valid,
                       int ncls, int topk, long long* acc, hipStream_t stream);
int sl_eval_accum(const float* logits, int ld, const uint8_t* lab, const float* loss_rows, int rows, int n_valid,
                  int ncls, int topk, long long* acc, hipStream_t stream);

// gossip_sparse.hip
long sl_gossip_topk_workspace(long n);
int sl_gossip_topk(const float* m, float* o, long n, long k, uint32_t* index_out, float* value_out,
                   uint32_t* count_out, void* workspace, hipStream_t stream);
int sl_gossip_scatter(float* m, float* o, const uint32_t* index, const float* value, long count, long n, double a,
                      int sign_o_only, hipStream_t stream);

// mlp_fused.hip
long sl_mlp_x_tile_bytes(long rows);
int sl_mlp_x_tile(const uint8_t* src, uint8_t* dst, long rows, hipStream_t stream);
long sl_mlp_param_count();
long sl_mlp_slab_stride();
int sl_mlp_set_stamps(unsigned long long* p);
int sl_mlp_set_sgd_stamps(unsigned long long* p);
int sl_mlp_sgd_wgs();
int sl_mlp_set_wg_stamps(unsigned long long* p);
int sl_mlp_wg_stamps();
int sl_mlp_set_wg_wide(int on);
int sl_mlp_set_rows_bm(int bm);
int sl_mlp_rows_bm(int batch);
int sl_mlp_rows(const uint8_t* x, const uint8_t* y, const int* cursor, int n_batches, int batch, const uint16_t* w1h,
                const uint16_t* w2h, const uint16_t* w3h, const uint16_t* w2th, const uint16_t* w3th,
                const float* params, float xa, float xb, float grad_scale, float dh1_scale, uint16_t* h1, float* w3p,
                uint16_t* dh2, uint16_t* dh1, float* loss, float* correct, float* logits, int train,
                const long long* r1p, unsigned* step_ctr, hipStream_t stream);
int sl_mlp_rows_xt(const uint8_t* x, const uint8_t* y, const int* cursor, int n_batches, int batch,
                   const uint16_t* w1h, const uint16_t* w2h, const uint16_t* w3h, const uint16_t* w2th,
                   const uint16_t* w3th, const float* params, float xa, float xb, float grad_scale, float dh1_scale,
                   uint16_t* h1, float* w3p, uint16_t* dh2, uint16_t* dh1, float* loss, float* correct, float* logits,
                   int train, const long long* r1p, unsigned* step_ctr, hipStream_t stream);
int sl_mlp_wgrad_slices(int batch, int requested);
int sl_mlp_wgrad(int batch, const uint8_t* x, const int* cursor, int n_batches, const uint16_t* h1,
                 const uint16_t* dh2, const uint16_t* dh1, const float* w3p, int n_w3p, float* slab, int slices,
                 long slab_stride, hipStream_t stream);
int sl_mlp_wgrad_xt(int batch, const uint8_t* x, const int* cursor, int n_batches, const uint16_t* h1,
                    const uint16_t* dh2, const uint16_t* dh1, const float* w3p, int n_w3p, float* slab, int slices,
                    long slab_stride, hipStream_t stream);
int sl_mlp_sgd(float* w, float* mom, const float* slab, int slices, long slab_stride, const float* grad_in,
               float* grad_out, float lr, float mu, float wd, float xa, float xb, int mode, uint16_t* w1h,
               uint16_t* w2h, uint16_t* w2th, uint16_t* w3h, uint16_t* w3th, int* cursor, long long* r1p,
               hipStream_t stream);
int sl_mlp_opt(int rule, float* w, float* mom, float* v, const float* slab, int slices, long slab_stride,
               const float* grad_in, float lr, float mu, float wd, float xa, float xb, uint16_t* w1h, uint16_t* w2h,
               uint16_t* w2th, uint16_t* w3h, uint16_t* w3th, int* cursor, long long* r1p, int* step,
               unsigned* ticket, const float* lr_tab, int lr_n, float b1, float b2, float omb1, float omb2,
               float lnb1, float lnb2, float eps, hipStream_t stream);
int sl_mlp_opt_groups(int rule, float* w, float* mom, float* v, const float* slab, int slices, long slab_stride,
                      const float* grad_in, float lr, float mu, float wd, float xa, float xb, uint16_t* w1h,
                      uint16_t* w2h, uint16_t* w2th, uint16_t* w3h, uint16_t* w3th, int* cursor, long long* r1p,
                      int* step, unsigned* ticket, const float* lr_tab, int lr_n, float b1, float b2, float omb1,
                      float omb2, float lnb1, float lnb2, float eps, float wd_bias, hipStream_t stream);
int sl_mlp_reduce_xgmi(const float* slab, int slices, long slab_stride, float xa, float xb, float* slot0,
                       float* slot1, char* const* bases, unsigned* ctl, long slot_bytes, int rank, int world,
                       long chunk4, int inline_sync, hipStream_t stream);
int sl_mlp_sgd_xgmi(float* w, float* mom, float lr, float mu, float wd, uint16_t* w1h, uint16_t* w2h, uint16_t* w2th,
                    uint16_t* w3h, uint16_t* w3th, int* cursor, char* const* bases, unsigned* ctl, long slot_bytes,
                    int rank, int world, long chunk4, long long* r1p, int inline_sync, hipStream_t stream);
int sl_mlp_opt_xgmi(int rule, float* w, float* mom, float* v, float lr, float mu, float wd, uint16_t* w1h,
                    uint16_t* w2h, uint16_t* w2th, uint16_t* w3h, uint16_t* w3th, int* cursor, char* const* bases,
                    unsigned* ctl, long slot_bytes, int rank, int world, long chunk4, long long* r1p, int inline_sync,
                    int* step, unsigned* ticket, const float* lr_tab, int lr_n, float b1, float b2, float omb1,
                    float omb2, float lnb1, float lnb2, float eps, hipStream_t stream);
int sl_mlp_opt_xgmi_groups(int rule, float* w, float* mom, float* v, float lr, float mu, float wd, uint16_t* w1h,
                           uint16_t* w2h, uint16_t* w2th, uint16_t* w3h, uint16_t* w3th, int* cursor,
                           char* const* bases, unsigned* ctl, long slot_bytes, int rank, int world, long chunk4,
                           long long* r1p, int inline_sync, int* step, unsigned* ticket, const float* lr_tab,
                           int lr_n, float b1, float b2, float omb1, float omb2, float lnb1, float lnb2, float eps,
                           float wd_bias, hipStream_t stream);

// xgmi.hip
int sl_xgmi_header_bytes();
long sl_xgmi_buffer_bytes(long slot_bytes);
int sl_xgmi_alloc(long bytes, void** out);
int sl_xgmi_free(void* p);
int sl_ipc_get_handle(void* p, void* handle_out);
int sl_ipc_handle_size();
int sl_ipc_open(const void* handle, void** out);
int sl_ipc_close(void* p);
int sl_xgmi_copyin(char* const* bases, unsigned* ctl, long slot_bytes, int rank, int world, long chunk4,
                   const float* src, long n, hipStream_t stream);
int sl_xgmi_barrier(char* const* bases, unsigned* ctl, long slot_bytes, int rank, int world, long chunk4, int set,
                    hipStream_t stream);
int sl_xgmi_rs(char* const* bases, unsigned* ctl, long slot_bytes, int rank, int world, long chunk4, long n,
               int inline_sync, hipStream_t stream);
int sl_xgmi_abort(unsigned* ctl, hipStream_t stream);
int sl_xgmi_sum(char* const* bases, unsigned* ctl, long slot_bytes, int rank, int world, long chunk4, float* out,
                long n, float scale, hipStream_t stream);
int sl_xgmi_peek(char* const* bases, unsigned* ctl, long slot_bytes, int rank, int world, long chunk4, int q,
                 int parity, int mode, float* out, long n, hipStream_t stream);

}  // extern "C"
