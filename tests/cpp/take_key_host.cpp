/*
 * take_key_host.cpp -- TEST-ONLY CPU build of carnd-mpc-project_amd/csrc/mpc_take_key.h: the take-order key of the bulk
 * launch (features and bin) and the binning the key kernel does with it, on struct-of-arrays inputs like the ABI's.
 * Used by tests/test_take_order.py and tools/take_order_model.py; never linked into the product library.
 */
#include <cstdint>

#include "mpc_take_key.h"

extern "C" int mpc_take_key_bins_n(void) { return mpc::kTakeBins; }
extern "C" int mpc_take_key_feats_n(void) { return mpc::kTakeFeats; }

/* feat: [B][kTakeFeats] or NULL; bins: [B] or NULL */
extern "C" void mpc_take_key_host(double horizon_s, int64_t B, int64_t ld, const double *state, const double *coeffs, const double *yaw_lo,
                                  const double *yaw_hi, float *feat, int32_t *bins) {
  for (int64_t i = 0; i < B; i++) {
    double st[6], cf[5];
    float f[mpc::kTakeFeats];
    for (int q = 0; q < 6; q++) st[q] = state[q * ld + i];
    for (int q = 0; q < 5; q++) cf[q] = coeffs[q * ld + i];
    mpc::take_key_features<double>((float)horizon_s, st, cf, yaw_lo[i], yaw_hi[i], f);
    if (feat) for (int q = 0; q < mpc::kTakeFeats; q++) feat[i * mpc::kTakeFeats + q] = f[q];
    if (bins) bins[i] = mpc::take_key_bin(f);
  }
}

/* what the key kernel leaves behind: cnt[kTakeBins] and list[kTakeBins][ld_list], entries in instance order within a bin */
extern "C" void mpc_take_key_lists_host(double horizon_s, int64_t B, int64_t ld, const double *state, const double *coeffs,
                                        const double *yaw_lo, const double *yaw_hi, int reverse, int64_t ld_list, int32_t *cnt, int32_t *list) {
  for (int b = 0; b < mpc::kTakeBins; b++) cnt[b] = 0;
  for (int64_t i = 0; i < B; i++) {
    int32_t b;
    mpc_take_key_host(horizon_s, 1, ld, state + i, coeffs + i, yaw_lo + i, yaw_hi + i, nullptr, &b);
    if (reverse) b = mpc::kTakeBins - 1 - b;
    list[(int64_t)b * ld_list + cnt[b]++] = (int32_t)i;
  }
}
