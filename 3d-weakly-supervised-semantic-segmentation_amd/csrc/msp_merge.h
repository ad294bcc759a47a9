// Shared by msp_merge.hip and msp_elastic.hip: the per-sample parameters, the membership test of a ball, the
// fp64 transform and the order-preserving map used by the atomic min / max of the batch assembly.
#pragma once
#include "msp_common.h"

#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace msp {

constexpr int kMT = 256;
constexpr int kMIt = 4;  // points per thread
constexpr int kMPB = kMT * kMIt;

struct MergeParams {
  const double* rot;   // [B][9]  row-major 3x3 (points are row vectors: t = a . rot)
  const double* c1;    // [B][3]
  const double* c2;    // [B][3]
  const double* u1;    // [B][3]  the two rand(3) draws of the offset
  const double* u2;    // [B][3]
  const float* shift;  // [B][3]  colour shift
};

// The ball of sample b (kBall only): the scene it is cut from, its centre, the squared radius.
struct BallParams {
  const int* scene_of;   // [B]
  const double* centre;  // [B][3]
  double r2;
};

// One rounding per product and per sum.  Written with plain operators under this file's `fp contract(off)`:
// the toolchain's __dmul_rn / __dadd_rn are inline functions of a header compiled under its own contraction
// setting, and a product of theirs that feeds a sum is fused into one FMA.  A member test on the ball's surface
// must not depend on that, so the distance uses these.
__device__ inline double mul_rn(double a, double b) { return a * b; }
__device__ inline double add_rn(double a, double b) { return a + b; }

// query_radius' reduced-distance test for the Euclidean metric, in the restatement's evaluation order
__device__ inline bool in_ball(double x, double y, double z, double cx, double cy, double cz, double r2) {
  const double dx = add_rn(x, -cx), dy = add_rn(y, -cy), dz = add_rn(z, -cz);
  return add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)) <= r2;
}

template <bool kBall>
__device__ inline int sample_scene(const BallParams& Q, int b) {
  if constexpr (kBall) return Q.scene_of[b];
  else return b;
}

template <bool kBall>
__device__ inline bool member(const float* __restrict__ xyz, int64_t i, const BallParams& Q, int b) {
  if constexpr (kBall)
    return in_ball((double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], Q.centre[3 * b],
                   Q.centre[3 * b + 1], Q.centre[3 * b + 2], Q.r2);
  else
    return true;
}

// order-preserving map of doubles onto int64 (for atomic min / max)
__device__ inline long long ord_of(double d) {
  long long i = __double_as_longlong(d);
  return i >= 0 ? i : (i ^ 0x7fffffffffffffffll);
}
__host__ __device__ inline double dbl_of(long long i) {
  const long long j = i >= 0 ? i : (i ^ 0x7fffffffffffffffll);
#ifdef __HIP_DEVICE_COMPILE__
  return __longlong_as_double(j);
#else
  double d;
  __builtin_memcpy(&d, &j, sizeof d);
  return d;
#endif
}

__device__ inline void transform(const float* __restrict__ xyz, int64_t i, const double* r, const double* c1,
                                 const double* c2, double (&t)[3]) {
  const double a0 = (double)xyz[3 * i], a1 = (double)xyz[3 * i + 1], a2 = (double)xyz[3 * i + 2];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double v = __dadd_rn(__dadd_rn(__dmul_rn(a0, r[j]), __dmul_rn(a1, r[3 + j])), __dmul_rn(a2, r[6 + j]));
    v = __dadd_rn(v, c1[j]);
    t[j] = __dadd_rn(v, c2[j]);
  }
}

// The workspace of msp_merge (msp_merge_workspace_size bytes), carved.
struct MergeWs {
  long long* mm;         // [B][6] ord_of(min), ord_of(max) of the placed coordinates
  double* offset;        // [B][3]
  unsigned* label_mask;  // [B]
  int64_t *counts, *starts, *total;
  void* sws;  // scan workspace
  int64_t nbx, m;
};
MergeWs merge_carve(void* ws, int B, int64_t max_scene_points);

// msp_merge_elastic's ends (msp_merge.hip): merge_begin sets mm / label_mask to their identities; merge_tail_elastic
// runs offset / count / scan / write / finish reading each point's t from D[(b * nbx * kMPB + (i - s0)) * 3 + j]
// instead of transforming it (Q.scene_of == nullptr: whole scenes).
void merge_begin(const MergeWs& W, int B, hipStream_t s);
int merge_tail_elastic(const char* what, const float* xyz, const float* rgb, const int64_t* labels,
                       const int64_t* scene_start, int B, double full_scale, MergeParams P, BallParams Q,
                       const double* D, int n_classes, int64_t* coords, float* feats, int64_t* labels_out,
                       int64_t* point_ids, int64_t point_id_base, int64_t* batch_offsets, float* scene_labels,
                       const MergeWs& W, hipStream_t s);

}  // namespace msp
