// Elastic distortion inside the device batch assembly (`elastic_deformation: True`, dataset/data.py:171-173;
// dataset/dataset_utils/data_processing.py:8-21): between the rotation and the random offset every training
// sample is displaced by two smooth random fields,
//
//   t1 = t  + g1(t)  * mag1,   gran1 = 6*scale//50,  mag1 = 40*scale/50
//   t2 = t1 + g2(t1) * mag2,   gran2 = 20*scale//50, mag2 = 160*scale/50
//
// where g is the trilinear interpolation of three grids of Gaussian noise (one per component, nodes 2*gran apart,
// bb_j = int32(max |x_j|) // gran + 3 nodes on axis j) blurred six times with a 3-tap box.  The specification is
// wsss3d/elastic.py; this file follows it operation by operation in fp64 with every product and sum rounded
// separately, so the batch is bitwise the restatement's.
//
// The noise is drawn on the host at a data-independent shape cap >= bb (wsss3d/elastic.py: elastic_caps) and the
// field uses the [:bb0, :bb1, :bb2] corner of it at cap strides; bb is computed here, so nothing is read back in
// the middle of a batch.  Passes of msp_merge_elastic, all on the caller's stream:
//
//   1. t = transform(a) -> D, abs-max of t per sample (atomic max on the bits of |t|) -> bb1 (clamped to cap1)
//   2. blur of field 1: six launches ping-ponging two workspace grids; cells at or beyond bb read as zero
//   3. t1 = t + g1(t) * mag1 -> D in place, abs-max of t1 -> bb2
//   4. blur of field 2
//   5. t2 = t1 + g2(t1) * mag2 -> D in place, min/max of t2 -> mm
//   6. msp_merge's offset / count / scan / write / finish with t read from D (merge_tail_elastic)
//
// D holds 3 doubles per point at row b * nbx * kMPB + (i - s0): indexed by the sample, not the scene, so two
// balls cut from one scene do not collide.  The interpolation keeps points on lanes and the three components in
// registers; its eight 4-byte reads per component hit a grid of a few hundred KB that stays in L2.
//
// status (device int, zeroed here): bit 0 = a bb was clamped to its cap (the caller's bound was wrong; every
// index stays in range, the field is not the specification's), bit 1 = a sample's cap / cell offsets are
// inconsistent (its fields are skipped).
#include "msp_merge.h"

#pragma clang fp contract(off)

namespace msp {

struct FieldParams {
  const float* grid;         // blurred noise: sample b, component c at 3 * cell_off[b] + c * cap0*cap1*cap2
  const int64_t* cell_off;   // [B+1]
  const int* cap;            // [B][3]
  const int* bb;             // [B][3]
  int gran;
  double mag;
};

__device__ inline double lerp_rn(double a, double b, double f) {
  return add_rn(mul_rn(a, add_rn(1.0, -f)), mul_rn(b, f));
}

// t += g(t) * mag for sample b.  i_j <= bb_j - 2 <= cap_j - 2, so every read is inside the sample's cap block.
__device__ inline void displace(const FieldParams& F, int b, double (&t)[3]) {
  const int* bb = F.bb + 3 * b;
  if (bb[0] < 2) return;  // inconsistent caps (status bit 1): no field
  const int64_t c1 = F.cap[3 * b + 1], c2 = F.cap[3 * b + 2], ncap = (int64_t)F.cap[3 * b] * c1 * c2;
  const double gran = (double)F.gran, step = mul_rn(2.0, gran);
  int64_t idx[3];
  double f[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double u = add_rn(t[j], mul_rn((double)(bb[j] - 1), gran)) / step;
    const double fl = floor(u), top = (double)(bb[j] - 2);
    const double i = !(fl >= 0.0) ? 0.0 : (fl > top ? top : fl);  // NaN -> 0
    idx[j] = (int64_t)i;
    f[j] = add_rn(u, -i);
  }
  const float* g = F.grid + 3 * F.cell_off[b] + (idx[0] * c1 + idx[1]) * c2 + idx[2];
  double v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c, g += ncap) {
    const double z00 = lerp_rn((double)g[0], (double)g[1], f[2]);
    const double z01 = lerp_rn((double)g[c2], (double)g[c2 + 1], f[2]);
    const double z10 = lerp_rn((double)g[c1 * c2], (double)g[c1 * c2 + 1], f[2]);
    const double z11 = lerp_rn((double)g[(c1 + 1) * c2], (double)g[(c1 + 1) * c2 + 1], f[2]);
    v[c] = lerp_rn(lerp_rn(z00, z01, f[1]), lerp_rn(z10, z11, f[1]), f[0]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = add_rn(t[c], mul_rn(v[c], F.mag));
}

// kStage 0: t = transform(a) -> D, abs-max -> amax.  1: D += field, abs-max -> amax.  2: D += field, min/max -> mm.
template <bool kBall, int kStage>
__global__ __launch_bounds__(kMT) void elastic_point_kernel(const float* __restrict__ xyz,
                                                            const int64_t* __restrict__ sstart, MergeParams P,
                                                            BallParams Q, FieldParams F, double* __restrict__ D,
                                                            long long* __restrict__ amax /*[B][3]*/,
                                                            long long* __restrict__ mm /*[B][6]*/) {
  __shared__ long long red[6][kMT / 64];
  const int b = blockIdx.y, sc = sample_scene<kBall>(Q, b);
  const int64_t s0 = sstart[sc], s1 = sstart[sc + 1];
  // abs-max: the bits of |t| order as the values do; 0 is the identity
  long long lo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX};
  long long hi[3] = {kStage == 2 ? LLONG_MIN : 0, kStage == 2 ? LLONG_MIN : 0, kStage == 2 ? LLONG_MIN : 0};
  for (int k = 0; k < kMIt; ++k) {
    const int64_t i = s0 + (int64_t)blockIdx.x * kMPB + k * kMT + threadIdx.x;
    if (i < s1 && member<kBall>(xyz, i, Q, b)) {
      double* d = D + 3 * (((int64_t)b * gridDim.x) * kMPB + (i - s0));
      double t[3];
      if constexpr (kStage == 0) {
        transform(xyz, i, P.rot + 9 * b, P.c1 + 3 * b, P.c2 + 3 * b, t);
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j) t[j] = d[j];
        displace(F, b, t);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        d[j] = t[j];
        if constexpr (kStage == 2) {
          lo[j] = min(lo[j], ord_of(t[j]));
          hi[j] = max(hi[j], ord_of(t[j]));
        } else {
          hi[j] = max(hi[j], (long long)__double_as_longlong(fabs(t[j])));
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      if constexpr (kStage == 2) lo[j] = min(lo[j], (long long)__shfl_xor(lo[j], d, 64));
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
    if constexpr (kStage == 2) {
      if (j < 3) atomicMin(&mm[6 * b + j], v);
      else atomicMax(&mm[6 * b + j], v);
    } else {
      if (j >= 3) atomicMax(&amax[3 * b + j - 3], v);
    }
  }
}

__global__ void elastic_init_kernel(long long* __restrict__ amax, int B, int* __restrict__ status) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < 6 * B) amax[e] = 0;  // both fields
  if (e == 0) *status = 0;
}

// bb[b][j] = min(int32(amax) / gran + 3, cap[b][j]) after checking that the sample's cap block lies inside the
// grids: every later index is derived from bb and cap, so nothing below can leave the workspace.
__global__ void elastic_bb_kernel(const long long* __restrict__ amax, const int* __restrict__ cap,
                                  const int64_t* __restrict__ cell_off, int B, int gran, int64_t cells_total,
                                  int* __restrict__ bb, int* __restrict__ status) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int64_t o0 = cell_off[b], o1 = cell_off[b + 1];
  const int64_t c0 = cap[3 * b], c1 = cap[3 * b + 1], c2 = cap[3 * b + 2];
  const bool ok = c0 >= 2 && c1 >= 2 && c2 >= 2 && o0 >= 0 && o0 <= o1 && o1 <= cells_total &&
                  (o1 - o0) / c2 >= c0 * c1;  // c0 * c1 * c2 <= o1 - o0 without overflow
  if (!ok) {
    bb[3 * b] = bb[3 * b + 1] = bb[3 * b + 2] = 0;
    atomicOr(status, 2);
    return;
  }
  for (int j = 0; j < 3; ++j) {
    const int a = (int)__longlong_as_double(amax[3 * b + j]);  // truncates; |t| >= 0
    long long q = (long long)(a / gran) + 3;
    const long long c = cap[3 * b + j];
    if (q > c) {
      q = c;
      atomicOr(status, 1);
    }
    bb[3 * b + j] = (int)q;
  }
}

// One pass of the 3-tap box along `axis` over the bb corner of every sample and component; one thread per cell
// of the cap layout (e indexes src and dst alike).  out = f32((l*w + c*w) + r*w), w = f64(f32(1)/f32(3)).
__global__ __launch_bounds__(256) void elastic_blur_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           const int64_t* __restrict__ cell_off,
                                                           const int* __restrict__ cap, const int* __restrict__ bb,
                                                           int B, int64_t n, int axis) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  int lo = 0, hi = B - 1;  // the last sample whose block starts at or before e
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (3 * cell_off[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  const int b = lo;
  const int b0 = bb[3 * b], b1 = bb[3 * b + 1], b2 = bb[3 * b + 2];
  if (b0 == 0) return;
  const int64_t c1 = cap[3 * b + 1], c2 = cap[3 * b + 2], ncap = (int64_t)cap[3 * b] * c1 * c2;
  const int64_t local = e - 3 * cell_off[b];
  if (local < 0 || local >= 3 * ncap) return;
  const int64_t r = local % ncap;
  const int64_t z = r % c2, y = (r / c2) % c1, x = r / (c2 * c1);
  if (x >= b0 || y >= b1 || z >= b2) return;
  const int64_t stride = axis == 0 ? c1 * c2 : (axis == 1 ? c2 : 1);
  const int64_t pos = axis == 0 ? x : (axis == 1 ? y : z), lim = axis == 0 ? b0 : (axis == 1 ? b1 : b2);
  const double w = (double)(1.0f / 3.0f);
  const double l = pos > 0 ? (double)src[e - stride] : 0.0, c = (double)src[e],
               u = pos + 1 < lim ? (double)src[e + stride] : 0.0;
  dst[e] = (float)add_rn(add_rn(mul_rn(l, w), mul_rn(c, w)), mul_rn(u, w));
}

struct ElasticWs {
  long long* amax;  // [2][B][3]
  int* bb;          // [2][B][3]
  float *g0, *g1;   // 3 * cap_cells_total each
  double* D;        // [B * nbx * kMPB][3]
};

inline size_t pad8(size_t n) { return (n + 7) / 8 * 8; }

inline size_t elastic_ws_bytes(int B, int64_t nbx, int64_t cells) {
  return (size_t)B * 6 * sizeof(long long) + pad8((size_t)B * 6 * sizeof(int)) +
         2 * pad8((size_t)cells * 3 * sizeof(float)) + (size_t)B * nbx * kMPB * 3 * sizeof(double);
}

template <bool kBall>
void elastic_launch(const float* xyz, const int64_t* scene_start, int B, MergeParams P, BallParams Q,
                    const float* const noise[2], const int* const cap[2], const int64_t* const cell_off[2],
                    int64_t cells, const int gran[2], const double mag[2], int* status, const MergeWs& W,
                    const ElasticWs& E, hipStream_t s) {
  const dim3 grid((unsigned)W.nbx, (unsigned)B);
  elastic_init_kernel<<<(unsigned)ceil_div(6 * B, 256), 256, 0, s>>>(E.amax, B, status);
  elastic_point_kernel<kBall, 0><<<grid, kMT, 0, s>>>(xyz, scene_start, P, Q, FieldParams{}, E.D, E.amax, W.mm);
  for (int f = 0; f < 2; ++f) {
    long long* amax = E.amax + (size_t)f * 3 * B;
    int* bb = E.bb + (size_t)f * 3 * B;
    elastic_bb_kernel<<<(unsigned)ceil_div(B, 64), 64, 0, s>>>(amax, cap[f], cell_off[f], B, gran[f], cells, bb,
                                                               status);
    if (cells > 0) {
      const int64_t n = 3 * cells;
      const float* src = noise[f];
      for (int pass = 0; pass < 6; ++pass) {  // noise -> g0 -> g1 -> g0 -> g1 -> g0 -> g1
        float* dst = (pass & 1) ? E.g1 : E.g0;
        elastic_blur_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, s>>>(src, dst, cell_off[f], cap[f], bb, B, n,
                                                                       pass % 3);
        src = dst;
      }
    }
    const FieldParams F{E.g1, cell_off[f], cap[f], bb, gran[f], mag[f]};
    if (f == 0)
      elastic_point_kernel<kBall, 1><<<grid, kMT, 0, s>>>(xyz, scene_start, P, Q, F, E.D, E.amax + 3 * B, W.mm);
    else
      elastic_point_kernel<kBall, 2><<<grid, kMT, 0, s>>>(xyz, scene_start, P, Q, F, E.D, nullptr, W.mm);
  }
}

}  // namespace msp

using namespace msp;

extern "C" {

size_t msp_merge_elastic_workspace_size(int B, int64_t max_scene_points, int64_t cap_cells_total) {
  if (B < 1 || cap_cells_total < 0) return 0;
  const int64_t nbx = ceil_div(max_scene_points > 0 ? max_scene_points : 1, kMPB);
  return pad8(msp_merge_workspace_size(B, max_scene_points)) + elastic_ws_bytes(B, nbx, cap_cells_total);
}

int msp_merge_elastic(const float* xyz, const float* rgb, const int64_t* labels, const int64_t* scene_start, int B,
                      int64_t max_scene_points, int mode, double full_scale, const double* rot, const double* c1,
                      const double* c2, const double* u1, const double* u2, const float* shift, int n_classes,
                      int64_t* coords, float* feats, int64_t* labels_out, int64_t* point_ids,
                      int64_t point_id_base, int64_t* batch_offsets, float* scene_labels, void* ws, size_t ws_bytes,
                      const int* scene_of, const double* centre, double r2, const float* noise1,
                      const float* noise2, const int* cap1, const int* cap2, const int64_t* cell_off1,
                      const int64_t* cell_off2, int64_t cap_cells_total, int gran1, double mag1, int gran2,
                      double mag2, int* status, msp_stream_t stream) {
  MSP_REQUIRE(B >= 1 && B <= 65535 && max_scene_points >= 0 && full_scale > 0 && n_classes >= 0,
              "msp_merge_elastic: bad arguments (B=%d max_scene_points=%lld)", B, (long long)max_scene_points);
  MSP_REQUIRE(mode == 0, "msp_merge_elastic: mode %d (only 0, train: valMerge has no elastic step)", mode);
  MSP_REQUIRE(n_classes <= 32, "msp_merge_elastic: n_classes=%d exceeds the 32-bit class mask", n_classes);
  MSP_REQUIRE(gran1 >= 1 && gran2 >= 1 && gran1 <= (1 << 24) && gran2 <= (1 << 24),
              "msp_merge_elastic: gran must be in [1, 2^24] (got %d, %d)", gran1, gran2);
  MSP_REQUIRE(std::isfinite(mag1) && std::isfinite(mag2), "msp_merge_elastic: mag must be finite (got %g, %g)", mag1,
              mag2);
  MSP_REQUIRE(noise1 && noise2 && cap1 && cap2 && cell_off1 && cell_off2,
              "msp_merge_elastic: noise, cap and cell offsets must not be null");
  MSP_REQUIRE(status, "msp_merge_elastic: status must not be null");
  MSP_REQUIRE((scene_of == nullptr) == (centre == nullptr),
              "msp_merge_elastic: scene_of and centre must both be given (balls) or both be null (whole scenes)");
  MSP_REQUIRE(!scene_of || (r2 > 0 && std::isfinite(r2)),
              "msp_merge_elastic: r2 must be positive and finite (got %g)", r2);
  MSP_REQUIRE(cap_cells_total >= 0 && cap_cells_total <= ((int64_t)1 << 30),
              "msp_merge_elastic: cap_cells_total=%lld out of range", (long long)cap_cells_total);
  MSP_REQUIRE(xyz && rgb && labels && scene_start && rot && c1 && c2 && u1 && u2 && shift && coords && feats &&
                  labels_out && batch_offsets && scene_labels && ws,
              "msp_merge_elastic: null argument");
  MSP_REQUIRE(ws_bytes >= msp_merge_elastic_workspace_size(B, max_scene_points, cap_cells_total),
              "msp_merge_elastic: workspace too small");
  hipStream_t s = as_stream(stream);
  const MergeWs W = merge_carve(ws, B, max_scene_points);
  char* w = static_cast<char*>(ws) + pad8(msp_merge_workspace_size(B, max_scene_points));
  ElasticWs E;
  E.amax = reinterpret_cast<long long*>(w);
  w += (size_t)B * 6 * sizeof(long long);
  E.bb = reinterpret_cast<int*>(w);
  w += pad8((size_t)B * 6 * sizeof(int));
  E.g0 = reinterpret_cast<float*>(w);
  w += pad8((size_t)cap_cells_total * 3 * sizeof(float));
  E.g1 = reinterpret_cast<float*>(w);
  w += pad8((size_t)cap_cells_total * 3 * sizeof(float));
  E.D = reinterpret_cast<double*>(w);
  const MergeParams P{rot, c1, c2, u1, u2, shift};
  const BallParams Q{scene_of, centre, r2};
  const float* const noise[2] = {noise1, noise2};
  const int* const cap[2] = {cap1, cap2};
  const int64_t* const cell_off[2] = {cell_off1, cell_off2};
  const int gran[2] = {gran1, gran2};
  const double mag[2] = {mag1, mag2};
  merge_begin(W, B, s);
  if (scene_of) elastic_launch<true>(xyz, scene_start, B, P, Q, noise, cap, cell_off, cap_cells_total, gran, mag,
                                     status, W, E, s);
  else elastic_launch<false>(xyz, scene_start, B, P, Q, noise, cap, cell_off, cap_cells_total, gran, mag, status, W,
                             E, s);
  return merge_tail_elastic("msp_merge_elastic", xyz, rgb, labels, scene_start, B, full_scale, P, Q, E.D, n_classes,
                            coords, feats, labels_out, point_ids, point_id_base, batch_offsets, scene_labels, W, s);
}

}  // extern "C"
