/* mpenv_policy_precision.h -- the precision of in-sim policy inference
 * (DESIGN.md §2 definitions 15 and 17).  Included by mpenv.h; callers include
 * that.
 *
 * A manager-wide switch.  MPENV_POLICY_F32, the default, is definition 15:
 * every value equals the reference's CPU network bit for bit.  With
 * MPENV_POLICY_BF16 the three trunk layers and the two heads run on the bf16
 * matrix cores under definition 17 -- dense inputs and weights rounded to
 * bf16 (round to nearest even), exact products, f32 accumulation in any order,
 * LayerNorm, logits and sampling in f32 -- several times faster and no longer
 * bit-equal to the reference.  The selection, the embed kernel, the slots,
 * the fallback to slot 0, the refusals and the RNG draws are the same.  It is
 * meant for frozen opponents; keep F32 for anything compared with the
 * reference bit for bit.
 *
 * Every loaded checkpoint holds both forms of its weights, so
 * mpenv_policy_set_precision may be called at any time, with or without a
 * checkpoint loaded; it takes effect with the next step, mpenv_policy_forward,
 * mpenv_policy_forward_slot or mpenv_debug_policy_step issued after it,
 * reloads nothing and leaves the captured step graph alone.  A value other
 * than the two below is MPENV_ERR_INVALID and mpenv_last_error names both.
 * mpenv_policy_precision reads the switch.
 *
 * mpenv_debug_policy_dense_bf16 (test hook): mpenv_debug_policy_dense through
 * the bf16 trunk's dense code: y[M][N] = bf16(x)[M][K] . bf16(w)[K][N], f32
 * accumulation; x, y in device memory, w_host in host memory, 1 <= K <= 512;
 * synchronous.
 * mpenv_debug_policy_pack_bf16 (test hook; needs no manager and no GPU):
 * w[K][N] rounded to bf16 in the B-operand order of
 * v_mfma_f32_32x32x16_bf16, K padded to a multiple of 16 and N to a multiple
 * of 32 with +0: element (((t * ceil(K / 16) + s) * 64 + l) * 8 + j) is
 * w[16 s + 8 (l >> 5) + j][32 t + (l & 31)].  *count receives the number of
 * 16-bit elements; with out null nothing else is written. */
#ifndef MPENV_POLICY_PRECISION_H
#define MPENV_POLICY_PRECISION_H

#include "mpenv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPENV_POLICY_F32 0
#define MPENV_POLICY_BF16 1

int mpenv_policy_set_precision(mpenv_manager *mgr, int32_t precision);
int mpenv_policy_precision(mpenv_manager *mgr, int32_t *out);
int mpenv_debug_policy_dense_bf16(mpenv_manager *mgr, const float *x_device, int32_t M, int32_t K,
                                  const float *w_host, int32_t N, float *y_device, void *hip_stream);
int mpenv_debug_policy_pack_bf16(const float *w, int32_t K, int32_t N, uint16_t *out, int64_t *count);

#ifdef __cplusplus
}
#endif

#endif /* MPENV_POLICY_PRECISION_H */
