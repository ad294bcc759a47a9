// Batch assembly on the device: the geometric part
// of the reference's DataLoader collate functions
//
//   trainMerge  dataset/data.py:135-238  (random scale/flip/rotation, random
//               offset into [0, full_scale)^3, crop, .long(), batch id in the
//               last column, per-scene colour shift, batch_offsets)
//   valMerge    dataset/data.py:256-310  (same with a centred placement and
//               per-point ids of the kept points)
//
// for B scenes whose raw points are already in HBM.  The random draws are
// data-independent and stay on the host (same numpy draw order as the
// restatement in wsss3d/synthetic.py); everything per point runs here.
//
// Arithmetic follows the numpy restatement operation by operation in fp64
// (no contraction into FMAs): t = ((a0*r0j + a1*r1j) + a2*r2j) + c1j + c2j,
// per-scene min/max of t, the offset formula of the mode, p = t + offset,
// keep = 0 <= p < full_scale, coordinate = trunc(p).  min/max are exact, so
// the atomic combination is order-independent; the compaction keeps the
// point order (block prefix sums), so the output is deterministic.
//
// Subcloud training (`label: subcloud`, data.py:69-125): a sample is the ball
// of radius in_radius around an anchor of a scene, not the scene.  The balls
// are never materialised: msp_merge_ball runs the same kernels with sample b
// reading scene scene_of[b] and the membership test
//   d2 = ((dx*dx + dy*dy) + dz*dz) <= r2,  dx = double(x) - centre_x
// (fp64, every product and sum rounded separately) fused into the three
// passes that read the points (min/max, count, stable write).  The kernels
// are templates on kBall; msp_merge instantiates kBall = false, in which the
// predicate is no code at all.  msp_ball_count counts the members of every
// anchor of every scene in one launch (integer LDS + global atomics: exact,
// order-independent); the host keeps the anchors with >= min_points members.
//
// Elastic distortion (msp_elastic.hip: msp_merge_elastic) displaces t before the placement and leaves it in a
// workspace D; the count and write kernels are templates on kElastic as well and then load t from D instead of
// transforming.  msp_merge and msp_merge_ball instantiate kElastic = false, in which D is never touched.
#include "msp_merge.h"

#pragma clang fp contract(off)

namespace msp {

template <bool kBall>
__global__ __launch_bounds__(kMT) void merge_minmax_kernel(const float* __restrict__ xyz,
                                                           const int64_t* __restrict__ sstart, MergeParams P,
                                                           BallParams Q, long long* __restrict__ mm /*[B][6]*/) {
  __shared__ long long red[6][kMT / 64];
  const int b = blockIdx.y, sc = sample_scene<kBall>(Q, b);
  const int64_t s0 = sstart[sc], s1 = sstart[sc + 1];
  long long lo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, hi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
  for (int k = 0; k < kMIt; ++k) {
    const int64_t i = s0 + (int64_t)blockIdx.x * kMPB + k * kMT + threadIdx.x;
    if (i < s1 && member<kBall>(xyz, i, Q, b)) {
      double t[3];
      transform(xyz, i, P.rot + 9 * b, P.c1 + 3 * b, P.c2 + 3 * b, t);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        lo[j] = min(lo[j], ord_of(t[j]));
        hi[j] = max(hi[j], ord_of(t[j]));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      lo[j] = min(lo[j], (long long)__shfl_xor(lo[j], d, 64));
      hi[j] = max(hi[j], (long long)__shfl_xor(hi[j], d, 64));
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int j = 0; j < 3; ++j) {
      red[j][wave] = lo[j];
      red[3 + j][wave] = hi[j];
    }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int j = threadIdx.x;
    long long v = red[j][0];
    for (int w = 1; w < kMT / 64; ++w) v = j < 3 ? min(v, red[j][w]) : max(v, red[j][w]);
    if (j < 3) atomicMin(&mm[6 * b + j], v);
    else atomicMax(&mm[6 * b + j], v);
  }
}

// offset[b] per the mode's formula (numpy evaluation order)
//   train (data.py:176-178): -m + clip(fs - (M - m) - 0.001, 0) * u1 + clip(fs - (M - m) + 0.001, None, 0) * u2
//   val   (data.py:273-275): -m + clip(fs - M + m - 0.001, 0) * u1 + clip(fs - M + m + 0.001, None, 0) * u2
__global__ void merge_offset_kernel(const long long* __restrict__ mm, int B, double fs, int mode, MergeParams P,
                                    double* __restrict__ offset) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 3 * B) return;
  const int b = e / 3, j = e % 3;
  if (mm[6 * b + j] > mm[6 * b + 3 + j]) {  // no point touched the identities (empty scene or ball): no NaN offset
    offset[e] = 0.0;
    return;
  }
  const double m = dbl_of(mm[6 * b + j]), M = dbl_of(mm[6 * b + 3 + j]);
  double q1, q2;
  if (mode == 0) {
    const double len = __dadd_rn(M, -m);
    q1 = __dadd_rn(__dadd_rn(fs, -len), -0.001);
    q2 = __dadd_rn(__dadd_rn(fs, -len), 0.001);
  } else {
    const double g = __dadd_rn(__dadd_rn(fs, -M), m);
    q1 = __dadd_rn(g, -0.001);
    q2 = __dadd_rn(g, 0.001);
  }
  q1 = q1 > 0.0 ? q1 : 0.0;
  q2 = q2 < 0.0 ? q2 : 0.0;
  offset[e] = __dadd_rn(__dadd_rn(-m, __dmul_rn(q1, P.u1[e])), __dmul_rn(q2, P.u2[e]));
}

// kElastic: the point's t was displaced by msp_merge_elastic and is read from D (row d) instead of transformed
template <bool kElastic>
__device__ inline bool kept(const float* __restrict__ xyz, int64_t i, int b, const MergeParams& P,
                            const double* __restrict__ D, int64_t d, const double* __restrict__ offset, double fs,
                            double (&p)[3]) {
  double t[3];
  if constexpr (kElastic) {
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = D[3 * d + j];
  } else {
    transform(xyz, i, P.rot + 9 * b, P.c1 + 3 * b, P.c2 + 3 * b, t);
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    p[j] = __dadd_rn(t[j], offset[3 * b + j]);
    ok = ok && p[j] >= 0.0 && p[j] < fs;
  }
  return ok;
}

// counts[b * nbx + bx] = kept points of block (b, bx)
template <bool kBall, bool kElastic>
__global__ __launch_bounds__(kMT) void merge_count_kernel(const float* __restrict__ xyz,
                                                          const int64_t* __restrict__ sstart, MergeParams P,
                                                          BallParams Q, const double* __restrict__ D,
                                                          const double* __restrict__ offset, double fs,
                                                          int64_t* __restrict__ counts) {
  const int b = blockIdx.y, sc = sample_scene<kBall>(Q, b);
  const int64_t s0 = sstart[sc], s1 = sstart[sc + 1];
  int64_t c = 0;
  for (int k = 0; k < kMIt; ++k) {
    const int64_t i = s0 + (int64_t)blockIdx.x * kMPB + k * kMT + threadIdx.x;
    double p[3];
    if (i < s1 && member<kBall>(xyz, i, Q, b) &&
        kept<kElastic>(xyz, i, b, P, D, ((int64_t)b * gridDim.x) * kMPB + (i - s0), offset, fs, p))
      ++c;
  }
  int64_t tot;
  block_excl_scan<kMT>(c, &tot);
  if (threadIdx.x == 0) counts[(int64_t)b * gridDim.x + blockIdx.x] = tot;
}

// stable compaction: output position = block start + prefix of the kept
// points in point order (thread-major inside each of the kMIt sweeps)
template <bool kBall, bool kElastic>
__global__ __launch_bounds__(kMT) void merge_write_kernel(const float* __restrict__ xyz,
                                                          const float* __restrict__ rgb,
                                                          const int64_t* __restrict__ lab_in,
                                                          const int64_t* __restrict__ sstart, MergeParams P,
                                                          BallParams Q, const double* __restrict__ D,
                                                          const double* __restrict__ offset, double fs,
                                                          const int64_t* __restrict__ starts,
                                                          int64_t* __restrict__ coords, float* __restrict__ feats,
                                                          int64_t* __restrict__ lab_out, int64_t* __restrict__ ids,
                                                          int64_t id_base, unsigned* __restrict__ label_mask) {
  const int b = blockIdx.y, sc = sample_scene<kBall>(Q, b);
  const int64_t s0 = sstart[sc], s1 = sstart[sc + 1];
  int64_t pos = starts[(int64_t)b * gridDim.x + blockIdx.x];
  unsigned mask = 0;
  for (int k = 0; k < kMIt; ++k) {
    const int64_t i = s0 + (int64_t)blockIdx.x * kMPB + k * kMT + threadIdx.x;
    double p[3];
    const bool keep = i < s1 && member<kBall>(xyz, i, Q, b) &&
                      kept<kElastic>(xyz, i, b, P, D, ((int64_t)b * gridDim.x) * kMPB + (i - s0), offset, fs, p);
    int64_t tot;
    const int64_t e = pos + block_excl_scan<kMT>((int64_t)keep, &tot);
    if (keep) {
      coords[4 * e + 0] = (int64_t)p[0];  // trunc toward zero (p >= 0): torch .long()
      coords[4 * e + 1] = (int64_t)p[1];
      coords[4 * e + 2] = (int64_t)p[2];
      coords[4 * e + 3] = b;
#pragma unroll
      for (int j = 0; j < 3; ++j) feats[3 * e + j] = rgb[3 * i + j] + P.shift[3 * b + j];
      const int64_t l = lab_in[i];
      lab_out[e] = l;
      if (l >= 0 && l < 32) mask |= 1u << l;
      if (ids) ids[e] = id_base + i;
    }
    pos += tot;
  }
  // scene label presence (data.py:188-191): OR is order-independent
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mask |= (unsigned)__shfl_xor((int)mask, d, 64);
  if ((threadIdx.x & 63) == 0 && mask) atomicOr(&label_mask[b], mask);
}

__global__ void merge_init_kernel(long long* __restrict__ mm, unsigned* __restrict__ label_mask, int B) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < 6 * B) mm[e] = (e % 6) < 3 ? LLONG_MAX : LLONG_MIN;  // identities of min (lo) and max (hi)
  if (e < B) label_mask[e] = 0u;
}

__global__ void merge_finish_kernel(const int64_t* __restrict__ starts, int nbx, int B,
                                    const int64_t* __restrict__ total, const unsigned* __restrict__ label_mask,
                                    int n_classes, int64_t* __restrict__ batch_offsets,
                                    float* __restrict__ scene_labels) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e <= B) batch_offsets[e] = e < B ? starts[(int64_t)e * nbx] : *total;
  if (e < B * n_classes) {
    const int b = e / n_classes, c = e % n_classes;
    scene_labels[e] = (label_mask[b] >> c) & 1u ? 1.f : 0.f;
  }
}

// ---- msp_ball_count: members of every anchor's ball, all scenes in one launch ------------------------------
// Block (bx, scene) holds kMPB points of the scene in registers and walks the scene's anchors in chunks of kBC
// centres staged in LDS, so any anchor count works.  Per anchor the block's members are counted with wave
// ballots, combined over the waves with an LDS integer atomic and over the blocks with one global integer
// atomic per (block, anchor with members): exact and independent of the order.
constexpr int kBC = 256;

__global__ void ball_zero_kernel(const int64_t* __restrict__ astart, int n_scenes,
                                 unsigned long long* __restrict__ counts) {
  const int64_t A = astart[n_scenes];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < A; e += (int64_t)gridDim.x * blockDim.x)
    counts[e] = 0ull;
}

__global__ __launch_bounds__(kMT) void ball_count_kernel(const float* __restrict__ xyz,
                                                         const int64_t* __restrict__ sstart,
                                                         const double* __restrict__ centres,
                                                         const int64_t* __restrict__ astart, double r2,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ double cen[3 * kBC];
  __shared__ unsigned cnt[kBC];
  const int sc = blockIdx.y;
  const int64_t s1 = sstart[sc + 1], base = sstart[sc] + (int64_t)blockIdx.x * kMPB;
  if (base >= s1) return;  // block-uniform: a scene shorter than the longest one
  double p[kMIt][3];
  bool live[kMIt];
#pragma unroll
  for (int k = 0; k < kMIt; ++k) {
    const int64_t i = base + k * kMT + threadIdx.x;
    live[k] = i < s1;
#pragma unroll
    for (int j = 0; j < 3; ++j) p[k][j] = live[k] ? (double)xyz[3 * i + j] : 0.0;
  }
  const int64_t a1 = astart[sc + 1];
  for (int64_t c0 = astart[sc]; c0 < a1; c0 += kBC) {
    const int nc = (int)(a1 - c0 < kBC ? a1 - c0 : kBC);
    for (int e = threadIdx.x; e < 3 * nc; e += kMT) cen[e] = centres[3 * c0 + e];
    for (int e = threadIdx.x; e < nc; e += kMT) cnt[e] = 0u;
    __syncthreads();
    for (int a = 0; a < nc; ++a) {
      const double cx = cen[3 * a], cy = cen[3 * a + 1], cz = cen[3 * a + 2];
      unsigned n = 0;
#pragma unroll
      for (int k = 0; k < kMIt; ++k)
        n += (unsigned)__popcll(ballot64(live[k] && in_ball(p[k][0], p[k][1], p[k][2], cx, cy, cz, r2)));
      if (lane_id() == 0 && n) atomicAdd(&cnt[a], n);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nc; e += kMT)
      if (cnt[e]) atomicAdd(&counts[c0 + e], (unsigned long long)cnt[e]);
    __syncthreads();  // cen / cnt are rewritten by the next chunk
  }
}

MergeWs merge_carve(void* ws, int B, int64_t max_scene_points) {
  MergeWs W;
  W.nbx = ceil_div(max_scene_points > 0 ? max_scene_points : 1, kMPB);
  W.m = (int64_t)B * W.nbx;
  char* w = static_cast<char*>(ws);
  W.mm = reinterpret_cast<long long*>(w);
  w += (size_t)B * 6 * sizeof(long long);
  W.offset = reinterpret_cast<double*>(w);
  w += (size_t)B * 3 * sizeof(double);
  W.label_mask = reinterpret_cast<unsigned*>(w);
  w += ((size_t)B * sizeof(unsigned) + 7) / 8 * 8;
  W.counts = reinterpret_cast<int64_t*>(w);
  W.starts = W.counts + W.m;
  W.total = W.starts + W.m;
  W.sws = W.total + 1;
  return W;
}

void merge_begin(const MergeWs& W, int B, hipStream_t s) {
  merge_init_kernel<<<(unsigned)ceil_div(6 * B, 256), 256, 0, s>>>(W.mm, W.label_mask, B);
}

// The passes after the per-sample min/max: offset, count, scan, stable write, finish.
template <bool kBall, bool kElastic>
int merge_tail(const char* what, const float* xyz, const float* rgb, const int64_t* labels,
               const int64_t* scene_start, int B, int mode, double full_scale, MergeParams P, BallParams Q,
               const double* D, int n_classes, int64_t* coords, float* feats, int64_t* labels_out,
               int64_t* point_ids, int64_t point_id_base, int64_t* batch_offsets, float* scene_labels,
               const MergeWs& W, hipStream_t s) {
  const dim3 grid((unsigned)W.nbx, (unsigned)B);
  merge_offset_kernel<<<(unsigned)ceil_div(3 * B, 64), 64, 0, s>>>(W.mm, B, full_scale, mode, P, W.offset);
  merge_count_kernel<kBall, kElastic><<<grid, kMT, 0, s>>>(xyz, scene_start, P, Q, D, W.offset, full_scale, W.counts);
  int rc = scan_exclusive_i64(W.counts, W.starts, W.m, W.total, W.sws, scan_ws_bytes(W.m), s);
  if (rc) return rc;
  merge_write_kernel<kBall, kElastic><<<grid, kMT, 0, s>>>(xyz, rgb, labels, scene_start, P, Q, D, W.offset,
                                                           full_scale, W.starts, coords, feats, labels_out,
                                                           point_ids, point_id_base, W.label_mask);
  const int nf = (B + 1) > B * n_classes ? B + 1 : B * n_classes;
  merge_finish_kernel<<<(unsigned)ceil_div(nf, 256), 256, 0, s>>>(W.starts, (int)W.nbx, B, W.total, W.label_mask,
                                                                  n_classes, batch_offsets, scene_labels);
  return check_launch(what);
}

int merge_tail_elastic(const char* what, const float* xyz, const float* rgb, const int64_t* labels,
                       const int64_t* scene_start, int B, double full_scale, MergeParams P, BallParams Q,
                       const double* D, int n_classes, int64_t* coords, float* feats, int64_t* labels_out,
                       int64_t* point_ids, int64_t point_id_base, int64_t* batch_offsets, float* scene_labels,
                       const MergeWs& W, hipStream_t s) {
  if (Q.scene_of)
    return merge_tail<true, true>(what, xyz, rgb, labels, scene_start, B, 0, full_scale, P, Q, D, n_classes, coords,
                                  feats, labels_out, point_ids, point_id_base, batch_offsets, scene_labels, W, s);
  return merge_tail<false, true>(what, xyz, rgb, labels, scene_start, B, 0, full_scale, P, Q, D, n_classes, coords,
                                 feats, labels_out, point_ids, point_id_base, batch_offsets, scene_labels, W, s);
}

// The launches of msp_merge (kBall = false) and msp_merge_ball (kBall = true); arguments already validated.
template <bool kBall>
int merge_launch(const char* what, const float* xyz, const float* rgb, const int64_t* labels,
                 const int64_t* scene_start, int B, int64_t max_scene_points, int mode, double full_scale,
                 MergeParams P, BallParams Q, int n_classes, int64_t* coords, float* feats, int64_t* labels_out,
                 int64_t* point_ids, int64_t point_id_base, int64_t* batch_offsets, float* scene_labels, void* ws,
                 hipStream_t s) {
  const MergeWs W = merge_carve(ws, B, max_scene_points);
  merge_begin(W, B, s);
  merge_minmax_kernel<kBall><<<dim3((unsigned)W.nbx, (unsigned)B), kMT, 0, s>>>(xyz, scene_start, P, Q, W.mm);
  return merge_tail<kBall, false>(what, xyz, rgb, labels, scene_start, B, mode, full_scale, P, Q, nullptr, n_classes,
                                  coords, feats, labels_out, point_ids, point_id_base, batch_offsets, scene_labels,
                                  W, s);
}

}  // namespace msp

using namespace msp;

extern "C" {

size_t msp_merge_workspace_size(int B, int64_t max_scene_points) {
  const int64_t nbx = ceil_div(max_scene_points > 0 ? max_scene_points : 1, kMPB);
  const int64_t m = (int64_t)B * nbx;
  return (size_t)B * 6 * sizeof(long long) + (size_t)B * 3 * sizeof(double) + (size_t)B * sizeof(unsigned) + 8 +
         (size_t)(2 * m + 1) * sizeof(int64_t) + scan_ws_bytes(m);
}

int msp_merge(const float* xyz, const float* rgb, const int64_t* labels, const int64_t* scene_start, int B,
              int64_t max_scene_points, int mode, double full_scale, const double* rot, const double* c1,
              const double* c2, const double* u1, const double* u2, const float* shift, int n_classes,
              int64_t* coords, float* feats, int64_t* labels_out, int64_t* point_ids, int64_t point_id_base,
              int64_t* batch_offsets, float* scene_labels, void* ws, size_t ws_bytes, msp_stream_t stream) {
  MSP_REQUIRE(B >= 1 && max_scene_points >= 0 && (mode == 0 || mode == 1) && full_scale > 0 && n_classes >= 0 &&
                  n_classes <= 32,
              "msp_merge: bad arguments (B=%d mode=%d n_classes=%d)", B, mode, n_classes);
  MSP_REQUIRE(ws_bytes >= msp_merge_workspace_size(B, max_scene_points), "msp_merge: workspace too small");
  return merge_launch<false>("msp_merge", xyz, rgb, labels, scene_start, B, max_scene_points, mode, full_scale,
                             MergeParams{rot, c1, c2, u1, u2, shift}, BallParams{nullptr, nullptr, 0.0}, n_classes,
                             coords, feats, labels_out, point_ids, point_id_base, batch_offsets, scene_labels, ws,
                             as_stream(stream));
}

size_t msp_merge_ball_workspace_size(int B, int64_t max_scene_points) {
  return msp_merge_workspace_size(B, max_scene_points);
}

int msp_merge_ball(const float* xyz, const float* rgb, const int64_t* labels, const int64_t* scene_start, int B,
                   int64_t max_scene_points, int mode, double full_scale, const double* rot, const double* c1,
                   const double* c2, const double* u1, const double* u2, const float* shift, int n_classes,
                   int64_t* coords, float* feats, int64_t* labels_out, int64_t* point_ids, int64_t point_id_base,
                   int64_t* batch_offsets, float* scene_labels, void* ws, size_t ws_bytes, const int* scene_of,
                   const double* centre, double r2, msp_stream_t stream) {
  MSP_REQUIRE(B >= 1 && B <= 65535 && max_scene_points >= 0 && full_scale > 0 && n_classes >= 0,
              "msp_merge_ball: bad arguments (B=%d max_scene_points=%lld)", B, (long long)max_scene_points);
  MSP_REQUIRE(mode == 0, "msp_merge_ball: mode %d (only 0, train, is built)", mode);
  MSP_REQUIRE(n_classes <= 32, "msp_merge_ball: n_classes=%d exceeds the 32-bit class mask", n_classes);
  MSP_REQUIRE(r2 > 0 && std::isfinite(r2), "msp_merge_ball: r2 must be positive and finite (got %g)", r2);
  MSP_REQUIRE(scene_of && centre, "msp_merge_ball: scene_of and centre must not be null");
  MSP_REQUIRE(ws_bytes >= msp_merge_ball_workspace_size(B, max_scene_points), "msp_merge_ball: workspace too small");
  return merge_launch<true>("msp_merge_ball", xyz, rgb, labels, scene_start, B, max_scene_points, mode, full_scale,
                            MergeParams{rot, c1, c2, u1, u2, shift}, BallParams{scene_of, centre, r2}, n_classes,
                            coords, feats, labels_out, point_ids, point_id_base, batch_offsets, scene_labels, ws,
                            as_stream(stream));
}

int msp_ball_count(const float* xyz, const int64_t* scene_start, int n_scenes, int64_t max_scene_points,
                   const double* centres, const int64_t* anchor_start, double r2, int64_t* counts,
                   msp_stream_t stream) {
  MSP_REQUIRE(n_scenes >= 1 && n_scenes <= 65535 && max_scene_points >= 0,
              "msp_ball_count: bad arguments (n_scenes=%d max_scene_points=%lld)", n_scenes,
              (long long)max_scene_points);
  MSP_REQUIRE(r2 > 0 && std::isfinite(r2), "msp_ball_count: r2 must be positive and finite (got %g)", r2);
  MSP_REQUIRE(xyz && scene_start && centres && anchor_start && counts, "msp_ball_count: null argument");
  hipStream_t s = as_stream(stream);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
  ball_zero_kernel<<<256, 256, 0, s>>>(anchor_start, n_scenes, out);
  const dim3 grid((unsigned)ceil_div(max_scene_points > 0 ? max_scene_points : 1, kMPB), (unsigned)n_scenes);
  ball_count_kernel<<<grid, kMT, 0, s>>>(xyz, scene_start, centres, anchor_start, r2, out);
  return check_launch("msp_ball_count");
}

}  // extern "C"
