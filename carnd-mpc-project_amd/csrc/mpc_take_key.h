/*
 * mpc_take_key.h -- the take-order key: which of kTakeBins bins of predicted work an instance belongs to.
 *
 * A wave of the bulk launch lives as long as the slowest of its 64 instances.  Handing the launch its instances bin by bin
 * makes the 64 instances of a wave need about the same number of passes.  The key is a function of what
 * the launch loads at take anyway -- state, road polynomial, psi bounds -- in fp32, no solver state, a few dozen flops:
 * ten features and a fixed binary tree of kTakeBins leaves over them.  Mirror images get the same key: everything is
 * flipped so that epsi0 >= 0 first.  What carries the prediction is how far the road's heading at the middle and at the end
 * of the horizon (x = v0 N dt / 2 and v0 N dt) lies outside the psi box: `under` alone has 60 % of the tree's importance.
 *
 * The tree is fitted by tools/take_order_model.py --fit (survey population, N = 10, PRNG streams the benchmark does not
 * use) and checked by it on held-out streams; leaves are numbered by predicted passes, bin 0 the hardest.  A wrong bin costs
 * time, never a result: the arithmetic of an instance does not depend on where in its launch it is taken.
 *
 * Plain C++: compiled for the device by mpc_solver.hip and for the host by tests/cpp/take_key_host.cpp.
 */
#ifndef MPC_TAKE_KEY_H
#define MPC_TAKE_KEY_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MPC_TK_HD __host__ __device__ __forceinline__
#else
#define MPC_TK_HD inline
#endif

namespace mpc {

constexpr int kTakeBins = 32;
constexpr int kTakeFeats = 10;
constexpr int kTakeNodes = kTakeBins - 1;

/* features: 0 v0, 1 |epsi0|, 2 cte0, 3 psi_lo, 4 psi_hi, 5 heading(L), 6 heading(L/2), 7 y(L/2), 8 over, 9 under -- after the flip */
template <class R>
MPC_TK_HD void take_key_features(float horizon_s, const R *st, const R *cf, R yaw_lo, R yaw_hi, float *f) {
  const float s = (float)st[5] < 0.0f ? -1.0f : 1.0f;
  const float lo = s < 0.0f ? -(float)yaw_hi : (float)yaw_lo, hi = s < 0.0f ? -(float)yaw_lo : (float)yaw_hi;
  const float c0 = s * (float)cf[0], c1 = s * (float)cf[1], c2 = s * (float)cf[2], c3 = s * (float)cf[3], c4 = s * (float)cf[4];
  const float v = (float)st[3], L = v * horizon_s, H = 0.5f * L;
  const float hL = atanf(c1 + L * (2.0f * c2 + L * (3.0f * c3 + L * (4.0f * c4))));
  const float hH = atanf(c1 + H * (2.0f * c2 + H * (3.0f * c3 + H * (4.0f * c4))));
  f[0] = v; f[1] = fabsf((float)st[5]); f[2] = s * (float)st[4]; f[3] = lo; f[4] = hi; f[5] = hL; f[6] = hH;
  f[7] = c0 + H * (c1 + H * (c2 + H * (c3 + H * c4)));
  f[8] = fmaxf(hL, hH) - hi;
  f[9] = lo - fminf(hL, hH);
}

/* node n: feature kTakeFeat[n] <= kTakeThr[n] ? kTakeKid[n][0] : kTakeKid[n][1]; a kid < 0 is the leaf of bin -1 - kid.
 * (A not-a-number feature compares false and goes right: every instance reaches a leaf.)  Kids point forward only. */
/* BEGIN FITTED TABLES (tools/take_order_model.py --fit) */
/* importance: under 0.61, psi_lo 0.12, heading_L 0.10, y_L2 0.08, abs_epsi0 0.03, over 0.02, heading_L2 0.01, cte0 0.01, v0 0.01, psi_hi 0.01 */
constexpr int8_t kTakeFeat[kTakeNodes] = {9, 3, 5, 1, 3, 9, 9, 1, 7, 0, 8, 3, 7, 5, 2, 4, 9, 9, 5, 7, 9, 9, 6, 6, 5, 0, 3, 9, 3, 6, 9};
constexpr float kTakeThr[kTakeNodes] = {-0.0153973717f, -0.236573249f, -1.54581189f, 0.629183054f, -0.616274953f, 0.196781069f, 0.00769524276f, 0.0999976471f, -1.77570629f, 20.332798f, -0.000164590776f, -0.737451911f, -13.1295815f, -1.5240407f, -4.65070915f, 0.289678514f, -0.0859682485f, -0.0463153757f, -0.180114746f, -3.48520255f, 0.1544227f, 0.282311738f, -0.176301509f, -1.19724226f, -1.50881863f, 21.3735218f, -0.466980278f, -0.049547296f, -0.162238687f, -0.576146066f, -0.0716136098f};
constexpr int8_t kTakeKid[kTakeNodes][2] = {{1, 2}, {7, 8}, {3, 4}, {20, -1}, {5, 6}, {11, 12}, {18, 19}, {-27, 13}, {9, 10}, {27, 28}, {14, 15}, {-29, 29}, {23, 24}, {-5, 16}, {-3, 17}, {-7, -23}, {25, 26}, {-28, -21}, {-20, -15}, {21, 22}, {-8, -2}, {-12, -16}, {-10, -6}, {-4, -13}, {-9, -19}, {-32, -31}, {-30, -26}, {-24, -17}, {-22, 30}, {-11, -25}, {-18, -14}};
/* mean passes (capped at the cut) of the fit's instances per bin: 19.4 17.3 16.7 16.2 15.8 15.8 15.3 15.2 15.0 15.0 15.0 14.8 14.6 14.5 14.5 14.1 14.0 13.9 13.0 13.0 12.9 12.4 12.4 12.3 12.2 12.1 12.0 11.9 11.8 11.2 11.1 10.6 */
/* END FITTED TABLES */

/* the walk, unrolled at compile time: features stay in registers, thresholds are literals, nothing is loaded */
template <int NODE>
MPC_TK_HD int take_key_walk(const float *f) {
  if constexpr (NODE < 0) return -1 - NODE;
  else return f[kTakeFeat[NODE]] <= kTakeThr[NODE] ? take_key_walk<kTakeKid[NODE][0]>(f) : take_key_walk<kTakeKid[NODE][1]>(f);
}
MPC_TK_HD int take_key_bin(const float *f) { return take_key_walk<0>(f); }

}  // namespace mpc
#endif
