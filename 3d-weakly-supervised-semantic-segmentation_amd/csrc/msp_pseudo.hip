// The pseudo-label stage on the device (pseudoLabelGeneration.py:46-59, utils/stats.py:5-48, utils/iou.py:19-22,
// utils/loss.py:29-33):
//
//   msp_pseudo_labels   mask, L2-normalise, sigmoid, max / first argmax, threshold, quality counts and the
//                       (label, gt) confusion in one pass over the (N, C) logits
//   msp_confusion       iou.confusion_matrix on device label vectors
//   msp_point_ce_*      cross entropy over the rows whose label is not -100, without the boolean gather:
//                       the kept count stays on the device, so the step can be captured into a graph
//   msp_voxel_ce_*      the same loss, and the adjoint of the scene mean of the logits, on the level-0 voxel rows:
//                       all points of a voxel share one logit row, so the log-sum-exp is taken once per voxel and
//                       a voxel's gradient row is (kept_v softmax_v - hist_v) / n_kept; no (N, C) tensor is formed
//
// The first three stream (N, C) f32 rows with C <= 64.  A tile of R = blockDim.x rows is contiguous in memory
// (R * C floats), so a block loads it with 16-byte loads in memory order and scatters it into an LDS image
// with an odd row stride; after the barrier lane t owns row t and walks its C columns conflict-free (odd
// stride: the 32 lanes of a half-wave sit on 32 different banks).  The CE backward writes its gradient tile
// into the same image and stores it back in memory order.  Counts are reduced per wave by ballot/popcount and
// leave a block as one 64-bit atomic per counter; confusion bins are counted in an LDS histogram and only the
// non-zero bins are flushed.  Every accumulated output is an integer, so results do not depend on the order
// in which blocks run.
#include "msp_common.h"

namespace msp {

constexpr int kMaxC = 64;          // classes (the reference has 20)
constexpr int kCePartials = 1024;  // stage-1 blocks of the CE loss sum (fixed: the sum's order is part of the result)
constexpr int kIgnore = -100;
constexpr int kMaxLd = 1024;      // row stride of the voxel rows: tile elements e * ld < 2^32 keep div_c exact

inline int tile_rows(int C) { return C <= 48 ? 256 : 128; }  // R * (C | 1) * 4 B  <=  50 KiB of LDS per block
inline int lds_stride(int C) { return C | 1; }
inline uint32_t div_magic(int C) { return C > 1 ? (uint32_t)(((1ull << 32) + (uint64_t)C - 1) / (uint64_t)C) : 0u; }
// e / C for e < 2^16, C <= 64 with magic = ceil(2^32 / C): exact, since e * (magic * C - 2^32) < 2^32
__device__ inline uint32_t div_c(uint32_t e, uint32_t magic) { return magic ? __umulhi(e, magic) : e; }

// persistent grid: as many blocks as are resident at once (160 KiB of LDS per CU, at most 7 blocks of 256 threads
// at these kernels' register counts), so no block waits for a slot and the per-block atomics stay few
inline unsigned stream_grid(int64_t n_tiles, size_t lds_bytes) {
  int64_t per_cu = (int64_t)((160u << 10) / (lds_bytes + 256));
  per_cu = per_cu > 7 ? 7 : (per_cu < 1 ? 1 : per_cu);
  const int64_t cap = (int64_t)device_cu_count() * per_cu;
  return (unsigned)(n_tiles < cap ? (n_tiles > 0 ? n_tiles : 1) : cap);
}

// rows [row0, row0 + nr) of src (N, C) -> tile[r * S + c]; vec: src is 16-byte aligned (row0 * C is a multiple of 4)
__device__ inline void stage_tile(const float* __restrict__ src, int64_t row0, int nr, int C, int S, uint32_t magic,
                                  bool vec, float* __restrict__ tile) {
  const float* p = src + row0 * C;
  const uint32_t nflt = (uint32_t)nr * (uint32_t)C;
  const uint32_t n4 = vec ? (nflt >> 2) : 0u;
  for (uint32_t q = threadIdx.x; q < n4; q += blockDim.x) {
    const float4 x = reinterpret_cast<const float4*>(p)[q];
    const float xs[4] = {x.x, x.y, x.z, x.w};
    uint32_t r = div_c(4u * q, magic);
    uint32_t c = 4u * q - r * (uint32_t)C;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      tile[r * S + c] = xs[k];
      if (++c == (uint32_t)C) { c = 0; ++r; }
    }
  }
  for (uint32_t e = 4u * n4 + threadIdx.x; e < nflt; e += blockDim.x) {
    const uint32_t r = div_c(e, magic);
    tile[r * S + (e - r * (uint32_t)C)] = p[e];
  }
}

// the reverse: tile -> rows [row0, row0 + nr) of dst
__device__ inline void unstage_tile(float* __restrict__ dst, int64_t row0, int nr, int C, int S, uint32_t magic,
                                    bool vec, const float* __restrict__ tile) {
  float* p = dst + row0 * C;
  const uint32_t nflt = (uint32_t)nr * (uint32_t)C;
  const uint32_t n4 = vec ? (nflt >> 2) : 0u;
  for (uint32_t q = threadIdx.x; q < n4; q += blockDim.x) {
    uint32_t r = div_c(4u * q, magic);
    uint32_t c = 4u * q - r * (uint32_t)C;
    float xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xs[k] = tile[r * S + c];
      if (++c == (uint32_t)C) { c = 0; ++r; }
    }
    reinterpret_cast<float4*>(p)[q] = make_float4(xs[0], xs[1], xs[2], xs[3]);
  }
  for (uint32_t e = 4u * n4 + threadIdx.x; e < nflt; e += blockDim.x) {
    const uint32_t r = div_c(e, magic);
    p[e] = tile[r * S + (e - r * (uint32_t)C)];
  }
}

__device__ inline void flush_hist(const int* __restrict__ hist, int bins, int64_t* __restrict__ out) {
  for (int k = threadIdx.x; k < bins; k += blockDim.x) {
    const int v = hist[k];
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(out + k), (unsigned long long)v);
  }
}

// dynamic LDS: [R * S] f32 tile, [4] int block counters, [C * C] int histogram (when confusion != NULL)
__global__ __launch_bounds__(256) void pseudo_labels_kernel(
    const float* __restrict__ logits, int64_t N, int C, uint32_t magic, int vec,
    const float* __restrict__ scene_labels, const int64_t* __restrict__ off, int B, float threshold,
    const int64_t* __restrict__ gt, int64_t* __restrict__ labels, float* __restrict__ conf_out,
    int64_t* __restrict__ counts, int64_t* __restrict__ confusion) {
  extern __shared__ float smem[];
  const int R = blockDim.x, S = C | 1, t = threadIdx.x;
  float* tile = smem;
  int* cnt = reinterpret_cast<int*>(smem + R * S);
  int* hist = cnt + 4;
  if (t < 4) cnt[t] = 0;
  if (confusion)
    for (int k = t; k < C * C; k += R) hist[k] = 0;
  const int64_t n_tiles = (N + R - 1) / R;
  for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const int64_t row0 = tl * R;
    const int nr = (int)(N - row0 < R ? N - row0 : R);
    __syncthreads();  // the previous tile's rows are consumed (first pass: the counters are zeroed)
    stage_tile(logits, row0, nr, C, S, magic, vec != 0, tile);
    // scene of the tile's first row: the last b in [0, B) with off[b] <= row0 (uniform, bounded by log2 B)
    int b = 0;
    for (int lo = 0, hi = B; hi - lo > 1;) {
      const int mid = (lo + hi) >> 1;
      if (off[mid] <= row0) b = lo = mid;
      else hi = mid;
    }
    __syncthreads();
    const int64_t i = row0 + t;
    bool in_scene = false, labelled = false, correct = false;
    if (t < nr) {
      while (b + 1 < B && off[b + 1] <= i) ++b;  // at most the scenes that start inside the tile
      in_scene = off[b] <= i && i < off[b + 1];
      float* x = tile + t * S;
      const float* sl = scene_labels + (int64_t)b * C;
      bool finite = true;
      float ss = 0.f;
#pragma unroll 4
      for (int c = 0; c < C; ++c) {  // the masked row replaces the row in LDS: the mask is read once
        const float v = x[c];
        finite = finite && isfinite(v);
        const float m = v * sl[c];
        x[c] = m;
        ss += m * m;
      }
      int64_t lab = kIgnore;
      float best = __builtin_nanf("");
      if (in_scene && finite) {
        // F.normalize: m / max(||m||, eps), as one reciprocal per row (a last-bit difference in v; equal m stay
        // equal and m = 0 stays 0, so ties and the exact 0.5 of a masked class are kept)
        const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
        int arg = 0;
        best = -1.f;
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
          const float s = 1.f / (1.f + expf(-(x[c] * inv)));  // masked classes: v = 0 -> exactly 0.5
          if (s > best) { best = s; arg = c; }                // strict: the first index of the maximum
        }
        if (!(best < threshold)) {
          lab = arg;
          labelled = true;
        }
      }
      labels[i] = lab;
      if (conf_out) conf_out[i] = best;
      if (labelled && gt) {
        const int64_t g = gt[i];
        correct = g == lab;
        if (confusion && g >= 0 && g < C) atomicAdd(&hist[(int)lab * C + (int)g], 1);
      }
    }
    const unsigned long long ml = ballot64(labelled), mc = ballot64(correct), mr = ballot64(in_scene);
    if ((t & 63) == 0) {
      if (ml) atomicAdd(&cnt[0], __popcll(ml));
      if (mc) atomicAdd(&cnt[1], __popcll(mc));
      if (mr) atomicAdd(&cnt[2], __popcll(mr));
    }
  }
  __syncthreads();
  if (t < 3 && cnt[t]) atomicAdd(reinterpret_cast<unsigned long long*>(counts + t), (unsigned long long)cnt[t]);
  if (confusion) flush_hist(hist, C * C, confusion);
}

__global__ __launch_bounds__(256) void confusion_kernel(const int64_t* __restrict__ pred,
                                                        const int64_t* __restrict__ gt, int64_t n, int C,
                                                        int64_t* __restrict__ confusion) {
  extern __shared__ float smem[];
  int* hist = reinterpret_cast<int*>(smem);
  for (int k = threadIdx.x; k < C * C; k += blockDim.x) hist[k] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = pred[i], g = gt[i];
    if (p >= 0 && p < C && g >= 0 && g < C) atomicAdd(&hist[(int)p * C + (int)g], 1);
  }
  __syncthreads();
  flush_hist(hist, C * C, confusion);
}

// sum of one double per thread over the block, in a fixed order: shuffle tree per wave, then the waves in order.
// Valid in thread 0.  red: one double per wave.
__device__ inline double block_sum_fixed(double v, double* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < nw; ++w) s += red[w];
  return s;
}

struct CePartial {
  double sum;
  int64_t kept, bad;
};

// stage 1: block p takes tiles p, p + P, ... in order; writes lse per row and its partial
__global__ __launch_bounds__(256) void point_ce_fwd_kernel(const float* __restrict__ logits, int64_t N, int C,
                                                           uint32_t magic, int vec,
                                                           const int64_t* __restrict__ labels,
                                                           float* __restrict__ lse_out,
                                                           CePartial* __restrict__ partial) {
  extern __shared__ float smem[];
  __shared__ double red[4];
  __shared__ int cnt[2];
  const int R = blockDim.x, S = C | 1, t = threadIdx.x;
  float* tile = smem;
  if (t < 2) cnt[t] = 0;
  double acc = 0.0;  // thread 0: the block's running sum
  int64_t kept = 0, bad = 0;
  const int64_t n_tiles = (N + R - 1) / R;
  for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const int64_t row0 = tl * R;
    const int nr = (int)(N - row0 < R ? N - row0 : R);
    __syncthreads();
    stage_tile(logits, row0, nr, C, S, magic, vec != 0, tile);
    __syncthreads();
    float term = 0.f;
    bool is_kept = false, is_bad = false;
    if (t < nr) {
      const float* x = tile + t * S;
      float mx = x[0];
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(x[c] - mx);
      const float lse = mx + logf(se);
      lse_out[row0 + t] = lse;
      const int64_t y = labels[row0 + t];
      is_kept = y >= 0 && y < C;  // never index with anything else
      is_bad = !is_kept && y != kIgnore;
      if (is_kept) term = lse - x[(int)y];
    }
    const unsigned long long mk = ballot64(is_kept), mb = ballot64(is_bad);
    if ((t & 63) == 0) {
      if (mk) atomicAdd(&cnt[0], __popcll(mk));
      if (mb) atomicAdd(&cnt[1], __popcll(mb));
    }
    const double s = block_sum_fixed((double)term, red);  // its barriers also order cnt[]
    if (t == 0) {
      acc += s;
      kept += cnt[0];
      bad += cnt[1];
      cnt[0] = cnt[1] = 0;
    }
  }
  if (t == 0) partial[blockIdx.x] = CePartial{acc, kept, bad};
}

// stage 2 (one block): the partials in a fixed order; loss = sum / kept (0 / 0 = NaN: torch's mean over nothing)
__global__ __launch_bounds__(256) void point_ce_final_kernel(const CePartial* __restrict__ partial, int P,
                                                             float* __restrict__ loss, int64_t* __restrict__ n_kept,
                                                             int64_t* __restrict__ n_bad) {
  __shared__ double red[4];
  __shared__ unsigned long long tot[2];
  const int t = threadIdx.x;
  if (t < 2) tot[t] = 0;
  double s = 0.0;
  int64_t k = 0, b = 0;
  for (int p = t; p < P; p += blockDim.x) {
    s += partial[p].sum;
    k += partial[p].kept;
    b += partial[p].bad;
  }
  const double sum = block_sum_fixed(s, red);  // its first barrier orders tot[]'s zeroing
  if (k) atomicAdd(&tot[0], (unsigned long long)k);
  if (b) atomicAdd(&tot[1], (unsigned long long)b);
  __syncthreads();
  if (t == 0) {
    const int64_t kept = (int64_t)tot[0];
    *loss = (float)(sum / (double)kept);
    *n_kept = kept;
    *n_bad = (int64_t)tot[1];
  }
}

__global__ __launch_bounds__(256) void point_ce_bwd_kernel(const float* __restrict__ logits, int64_t N, int C,
                                                           uint32_t magic, int vec_in, int vec_out,
                                                           const int64_t* __restrict__ labels,
                                                           const float* __restrict__ lse,
                                                           const int64_t* __restrict__ n_kept,
                                                           const float* __restrict__ gout,
                                                           float* __restrict__ dlogits) {
  extern __shared__ float smem[];
  const int R = blockDim.x, S = C | 1, t = threadIdx.x;
  float* tile = smem;
  const int64_t nk = *n_kept;
  const float scale = nk > 0 ? *gout / (float)nk : 0.f;  // no kept row: every row below is ignored anyway
  const int64_t n_tiles = (N + R - 1) / R;
  for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const int64_t row0 = tl * R;
    const int nr = (int)(N - row0 < R ? N - row0 : R);
    __syncthreads();
    stage_tile(logits, row0, nr, C, S, magic, vec_in != 0, tile);
    __syncthreads();
    if (t < nr) {
      float* x = tile + t * S;
      const int64_t y = labels[row0 + t];
      if (y >= 0 && y < C) {
        const float l = lse[row0 + t];
        for (int c = 0; c < C; ++c) x[c] = scale * (expf(x[c] - l) - (c == (int)y ? 1.f : 0.f));
      } else {
        for (int c = 0; c < C; ++c) x[c] = 0.f;
      }
    }
    __syncthreads();
    unstage_tile(dlogits, row0, nr, C, S, magic, vec_out != 0, tile);
  }
}

// ---------------------------------------------------------------- cross entropy on the voxel rows
// A tile is R = blockDim.x voxel rows of row stride ld >= C; z = row[:C] + bias is staged into the same LDS image
// as above (memory-order loads of the whole padded rows, columns >= C dropped), lane t owns voxel row0 + t: it
// takes the row's lse and walks the voxel's points perm[vstart[v] .. vstart[v+1]).  Neighbouring lanes walk
// neighbouring runs of perm, so those reads coalesce; the labels are an 8-byte gather in point order.  A voxel
// with more than kHeavyPoints points is not walked by its lane: the wave takes such voxels one after the other,
// 64 points per step, so a crowded voxel costs cnt / 64 dependent gathers instead of cnt.
constexpr int kHeavyPoints = 64;

__device__ inline void stage_voxel_tile(const float* __restrict__ vl, int64_t row0, int nr, int ld, int C, int S,
                                        uint32_t magic_ld, bool vec, const float* __restrict__ bias,
                                        float* __restrict__ tile) {
  const float* p = vl + row0 * ld;
  const uint32_t nflt = (uint32_t)nr * (uint32_t)ld;
  const uint32_t n4 = vec ? (nflt >> 2) : 0u;  // vec: ld % 4 == 0, so a float4 never straddles two rows
  for (uint32_t q = threadIdx.x; q < n4; q += blockDim.x) {
    const float4 x = reinterpret_cast<const float4*>(p)[q];
    const float xs[4] = {x.x, x.y, x.z, x.w};
    const uint32_t r = div_c(4u * q, magic_ld);
    const uint32_t c = 4u * q - r * (uint32_t)ld;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c + k < (uint32_t)C) tile[r * S + c + k] = bias ? xs[k] + bias[c + k] : xs[k];
  }
  for (uint32_t e = 4u * n4 + threadIdx.x; e < nflt; e += blockDim.x) {
    const uint32_t r = div_c(e, magic_ld);
    const uint32_t c = e - r * (uint32_t)ld;
    if (c < (uint32_t)C) tile[r * S + c] = bias ? p[e] + bias[c] : p[e];
  }
}

// label of the j-th point of the sorted order; anything that cannot be read is ignored
__device__ inline int64_t point_label(const int32_t* __restrict__ perm, const int64_t* __restrict__ labels,
                                      int64_t N, int64_t j) {
  const int64_t p = perm[j];
  return (p >= 0 && p < N) ? labels[p] : (int64_t)kIgnore;
}

// point run of voxel v, clamped to [0, N]
__device__ inline void point_run(const int32_t* __restrict__ vstart, int64_t v, int64_t N, int64_t& s, int64_t& e) {
  s = vstart[v];
  e = vstart[v + 1];
  s = s < 0 ? 0 : (s > N ? N : s);
  e = e < s ? s : (e > N ? N : e);
}

__device__ inline int wave_sum_int(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// stage 1: block p takes tiles p, p + P, ... in order; writes lse and the kept count per voxel and its partial
__global__ __launch_bounds__(256) void voxel_ce_fwd_kernel(const float* __restrict__ vl, int64_t V, int ld, int C,
                                                           uint32_t magic_ld, int vec,
                                                           const float* __restrict__ bias,
                                                           const int32_t* __restrict__ perm,
                                                           const int32_t* __restrict__ vstart,
                                                           const int64_t* __restrict__ labels, int64_t N,
                                                           float* __restrict__ lse_out, int32_t* __restrict__ kept_out,
                                                           CePartial* __restrict__ partial) {
  extern __shared__ float smem[];
  __shared__ double red[4];
  __shared__ int cnt[2];
  const int R = blockDim.x, S = C | 1, t = threadIdx.x, lane = t & 63;
  float* tile = smem;
  if (t < 2) cnt[t] = 0;
  double acc = 0.0;  // thread 0: the block's running sum
  int64_t kept = 0, bad = 0;
  const int64_t n_tiles = (V + R - 1) / R;
  for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const int64_t row0 = tl * R;
    const int nr = (int)(V - row0 < R ? V - row0 : R);
    __syncthreads();
    stage_voxel_tile(vl, row0, nr, ld, C, S, magic_ld, vec != 0, bias, tile);
    __syncthreads();
    double term = 0.0;
    int nk = 0, nb = 0;
    int64_t s = 0, e = 0;
    float lse = 0.f;
    bool heavy = false;
    if (t < nr) {
      const float* x = tile + t * S;
      float mx = x[0];
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(x[c] - mx);
      lse = mx + logf(se);
      lse_out[row0 + t] = lse;
      point_run(vstart, row0 + t, N, s, e);
      heavy = e - s > kHeavyPoints;
      if (!heavy) {
        for (int64_t j = s; j < e; ++j) {
          const int64_t y = point_label(perm, labels, N, j);
          if (y >= 0 && y < C) {  // never index with anything else
            term += (double)(lse - x[(int)y]);
            ++nk;
          } else if (y != kIgnore) {
            ++nb;
          }
        }
      }
    }
    for (unsigned long long hm = ballot64(heavy); hm; hm &= hm - 1) {  // wave-uniform
      const int src = __builtin_ctzll(hm);
      const int64_t hs = __shfl(s, src, 64), he = __shfl(e, src, 64);
      const float hl = __shfl(lse, src, 64);
      const float* x = tile + (t - lane + src) * S;
      double part = 0.0;
      int pk = 0, pb = 0;
      for (int64_t j = hs + lane; j < he; j += 64) {
        const int64_t y = point_label(perm, labels, N, j);
        if (y >= 0 && y < C) {
          part += (double)(hl - x[(int)y]);
          ++pk;
        } else if (y != kIgnore) {
          ++pb;
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);  // the same tree on every run
      pk = wave_sum_int(pk);
      pb = wave_sum_int(pb);
      if (lane == src) {
        term = part;
        nk = pk;
        nb = pb;
      }
    }
    if (t < nr) kept_out[row0 + t] = nk;
    const int wk = wave_sum_int(nk), wb = wave_sum_int(nb);
    if (lane == 0) {
      if (wk) atomicAdd(&cnt[0], wk);
      if (wb) atomicAdd(&cnt[1], wb);
    }
    const double sum = block_sum_fixed(term, red);  // its barriers also order cnt[]
    if (t == 0) {
      acc += sum;
      kept += cnt[0];
      bad += cnt[1];
      cnt[0] = cnt[1] = 0;
    }
  }
  if (t == 0) partial[blockIdx.x] = CePartial{acc, kept, bad};
}

// dynamic LDS: [R * S] f32 tile, [R] f32 scene weights cnt_v / n_b, [R] int scene of the row
__global__ __launch_bounds__(256) void voxel_ce_bwd_kernel(
    const float* vl, int64_t V, int ld, int C, uint32_t magic_ld, int vec_in, int vec_out,  // dvl may be vl
    const float* __restrict__ bias, const int32_t* __restrict__ perm, const int32_t* __restrict__ vstart,
    const int64_t* __restrict__ labels, int64_t N, const float* __restrict__ lse, const int32_t* __restrict__ kept,
    const int64_t* __restrict__ n_kept, const float* __restrict__ gout, const float* __restrict__ gscene,
    const uint64_t* __restrict__ keys, int shift, int B, const int64_t* __restrict__ npts, float* dvl) {
  extern __shared__ float smem[];
  const int R = blockDim.x, S = C | 1, t = threadIdx.x, lane = t & 63;
  float* tile = smem;
  float* rw = smem + R * S;
  int* rb = reinterpret_cast<int*>(rw + R);
  const int64_t nk = *n_kept;
  const float scale = nk > 0 ? *gout / (float)nk : 0.f;  // no kept point: the CE term is zero, not NaN
  const int64_t n_tiles = (V + R - 1) / R;
  for (int64_t tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
    const int64_t row0 = tl * R;
    const int nr = (int)(V - row0 < R ? V - row0 : R);
    __syncthreads();
    stage_voxel_tile(vl, row0, nr, ld, C, S, magic_ld, vec_in != 0, bias, tile);
    __syncthreads();
    int64_t s = 0, e = 0;
    bool heavy = false;
    if (t < nr) {
      float* x = tile + t * S;
      const int64_t v = row0 + t;
      const int k = nk > 0 ? kept[v] : 0;
      point_run(vstart, v, N, s, e);
      float w = 0.f;
      int b = 0;
      if (gscene) {
        const uint64_t kb = keys[v] >> shift;
        if (kb < (uint64_t)B) {
          b = (int)kb;
          const int64_t n = npts[b];
          w = n > 0 ? (float)(vstart[v + 1] - vstart[v]) / (float)n : 0.f;
        }
      }
      rw[t] = w;
      rb[t] = b;
      if (k > 0) {
        // kept_v softmax_v - hist_v, unscaled: the histogram is subtracted one point at a time (each step is
        // exact until the value passes -kept_v softmax_v, and rounds to a coarser grid at most once per binade)
        const float l = lse[v], fk = (float)k;
        for (int c = 0; c < C; ++c) x[c] = fk * expf(x[c] - l);
        heavy = e - s > kHeavyPoints;
        if (!heavy) {
          for (int64_t j = s; j < e; ++j) {
            const int64_t y = point_label(perm, labels, N, j);
            if (y >= 0 && y < C) x[(int)y] -= 1.f;
          }
        }
      } else {
        for (int c = 0; c < C; ++c) x[c] = 0.f;
      }
    }
    for (unsigned long long hm = ballot64(heavy); hm; hm &= hm - 1) {  // wave-uniform; lane c counts class c
      const int src = __builtin_ctzll(hm);
      const int64_t hs = __shfl(s, src, 64), he = __shfl(e, src, 64);
      int h = 0;
      for (int64_t j0 = hs; j0 < he; j0 += 64) {
        const int64_t j = j0 + lane;
        const int64_t y = j < he ? point_label(perm, labels, N, j) : (int64_t)kIgnore;
        const int yy = (y >= 0 && y < C) ? (int)y : -1;
        for (int c = 0; c < C; ++c) {
          const int n = __popcll(ballot64(yy == c));
          if (lane == c) h += n;
        }
      }
      if (lane < C) tile[(t - lane + src) * S + lane] -= (float)h;
    }
    __syncthreads();
    // rows [row0, row0 + nr) of dvl in memory order: scale * tile + w * gscene[b], columns C .. ld-1 zero
    float* p = dvl + row0 * ld;
    const uint32_t nflt = (uint32_t)nr * (uint32_t)ld;
    const uint32_t n4 = vec_out ? (nflt >> 2) : 0u;
    for (uint32_t q = t; q < n4; q += R) {
      const uint32_t r = div_c(4u * q, magic_ld);
      const uint32_t c = 4u * q - r * (uint32_t)ld;
      const float w = rw[r];
      const float* g = gscene ? gscene + (int64_t)rb[r] * C : nullptr;
      float xs[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t ck = c + k;
        xs[k] = ck < (uint32_t)C ? scale * tile[r * S + ck] + (g ? w * g[ck] : 0.f) : 0.f;
      }
      reinterpret_cast<float4*>(p)[q] = make_float4(xs[0], xs[1], xs[2], xs[3]);
    }
    for (uint32_t el = 4u * n4 + t; el < nflt; el += R) {
      const uint32_t r = div_c(el, magic_ld);
      const uint32_t c = el - r * (uint32_t)ld;
      p[el] = c < (uint32_t)C ? scale * tile[r * S + c] + (gscene ? rw[r] * gscene[(int64_t)rb[r] * C + c] : 0.f)
                              : 0.f;
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline size_t tile_lds(int C) { return (size_t)tile_rows(C) * lds_stride(C) * sizeof(float); }
inline int ce_partials(int64_t N, int C) {
  const int64_t n_tiles = ceil_div(N > 0 ? N : 0, tile_rows(C));
  return (int)(n_tiles < kCePartials ? n_tiles : kCePartials);
}

}  // namespace msp

using namespace msp;

extern "C" {

int msp_pseudo_labels(const float* logits, int64_t N, int C, const float* scene_labels, const int64_t* point_offsets,
                      int B, float threshold, const int64_t* gt, int64_t* labels, float* conf, int64_t* counts,
                      int64_t* confusion, msp_stream_t stream) {
  MSP_REQUIRE(C >= 1 && C <= kMaxC, "msp_pseudo_labels: C=%d outside [1, %d]", C, kMaxC);
  MSP_REQUIRE(N >= 0 && B >= 1, "msp_pseudo_labels: bad arguments (N=%lld B=%d)", (long long)N, B);
  if (N == 0) return MSP_OK;
  MSP_REQUIRE(!confusion || gt, "msp_pseudo_labels: a confusion matrix needs gt");
  MSP_REQUIRE(logits && scene_labels && point_offsets && labels && counts, "msp_pseudo_labels: NULL pointer");
  const int R = tile_rows(C);
  const size_t lds = tile_lds(C) + 4 * sizeof(int) + (confusion ? (size_t)C * C * sizeof(int) : 0);
  pseudo_labels_kernel<<<stream_grid(ceil_div(N, R), lds), R, lds, as_stream(stream)>>>(
      logits, N, C, div_magic(C), aligned16(logits) ? 1 : 0, scene_labels, point_offsets, B, threshold, gt, labels,
      conf, counts, confusion);
  return check_launch("msp_pseudo_labels");
}

int msp_confusion(const int64_t* pred, const int64_t* gt, int64_t n, int C, int64_t* confusion,
                  msp_stream_t stream) {
  MSP_REQUIRE(C >= 1 && C <= kMaxC, "msp_confusion: C=%d outside [1, %d]", C, kMaxC);
  MSP_REQUIRE(n >= 0, "msp_confusion: n=%lld", (long long)n);
  if (n == 0) return MSP_OK;
  MSP_REQUIRE(pred && gt && confusion, "msp_confusion: NULL pointer");
  confusion_kernel<<<stream_grid(ceil_div(n, 1024), 0), 256, (size_t)C * C * sizeof(int), as_stream(stream)>>>(
      pred, gt, n, C, confusion);
  return check_launch("msp_confusion");
}

size_t msp_point_ce_workspace_size(int64_t N) {
  const int64_t n_tiles = ceil_div(N > 0 ? N : 0, 128);  // the smaller tile: enough for every C
  return sizeof(CePartial) * (size_t)(n_tiles < kCePartials ? (n_tiles > 0 ? n_tiles : 1) : kCePartials);
}

int msp_point_ce_fwd(const float* logits, int64_t N, int C, const int64_t* labels, float* loss, int64_t* n_kept,
                     int64_t* n_bad, float* lse, void* ws, size_t ws_bytes, msp_stream_t stream) {
  MSP_REQUIRE(C >= 1 && C <= kMaxC, "msp_point_ce_fwd: C=%d outside [1, %d]", C, kMaxC);
  MSP_REQUIRE(N >= 0, "msp_point_ce_fwd: N=%lld", (long long)N);
  const size_t need = msp_point_ce_workspace_size(N);
  MSP_REQUIRE(ws_bytes >= need, "msp_point_ce_fwd: workspace too small (%zu < %zu)", ws_bytes, need);
  MSP_REQUIRE(loss && n_kept && n_bad && ws, "msp_point_ce_fwd: NULL pointer");
  MSP_REQUIRE(N == 0 || (logits && labels && lse), "msp_point_ce_fwd: NULL pointer");
  hipStream_t s = as_stream(stream);
  CePartial* partial = static_cast<CePartial*>(ws);
  const int P = ce_partials(N, C);
  if (P > 0)
    point_ce_fwd_kernel<<<P, tile_rows(C), tile_lds(C), s>>>(logits, N, C, div_magic(C), aligned16(logits) ? 1 : 0,
                                                             labels, lse, partial);
  point_ce_final_kernel<<<1, 256, 0, s>>>(partial, P, loss, n_kept, n_bad);
  return check_launch("msp_point_ce_fwd");
}

int msp_point_ce_bwd(const float* logits, int64_t N, int C, const int64_t* labels, const float* lse,
                     const int64_t* n_kept, const float* gout, float* dlogits, msp_stream_t stream) {
  MSP_REQUIRE(C >= 1 && C <= kMaxC, "msp_point_ce_bwd: C=%d outside [1, %d]", C, kMaxC);
  MSP_REQUIRE(N >= 0, "msp_point_ce_bwd: N=%lld", (long long)N);
  if (N == 0) return MSP_OK;
  MSP_REQUIRE(logits && labels && lse && n_kept && gout && dlogits, "msp_point_ce_bwd: NULL pointer");
  const int R = tile_rows(C);
  point_ce_bwd_kernel<<<stream_grid(ceil_div(N, R), tile_lds(C)), R, tile_lds(C), as_stream(stream)>>>(
      logits, N, C, div_magic(C), aligned16(logits) ? 1 : 0, aligned16(dlogits) ? 1 : 0, labels, lse, n_kept, gout,
      dlogits);
  return check_launch("msp_point_ce_bwd");
}

size_t msp_voxel_ce_workspace_size(int64_t V) { return msp_point_ce_workspace_size(V); }

int msp_voxel_ce_fwd(const float* vl, int64_t V, int64_t ld, int C, const float* bias, const int32_t* perm,
                     const int32_t* vstart, const int64_t* labels, int64_t N, float* loss, int64_t* n_kept,
                     int64_t* n_bad, float* lse, int32_t* kept, void* ws, size_t ws_bytes, msp_stream_t stream) {
  MSP_REQUIRE(C >= 1 && C <= kMaxC, "msp_voxel_ce_fwd: C=%d outside [1, %d]", C, kMaxC);
  MSP_REQUIRE(V >= 0 && N >= 0 && N < (1ll << 31) && ld >= C && ld <= kMaxLd,
              "msp_voxel_ce_fwd: bad arguments (V=%lld N=%lld ld=%lld)", (long long)V, (long long)N, (long long)ld);
  const size_t need = msp_voxel_ce_workspace_size(V);
  MSP_REQUIRE(ws_bytes >= need, "msp_voxel_ce_fwd: workspace too small (%zu < %zu)", ws_bytes, need);
  MSP_REQUIRE(loss && n_kept && n_bad && ws, "msp_voxel_ce_fwd: NULL pointer");
  MSP_REQUIRE(V == 0 || (vl && perm && vstart && labels && lse && kept), "msp_voxel_ce_fwd: NULL pointer");
  hipStream_t s = as_stream(stream);
  CePartial* partial = static_cast<CePartial*>(ws);
  const int P = ce_partials(V, C);
  if (P > 0)
    voxel_ce_fwd_kernel<<<P, tile_rows(C), tile_lds(C), s>>>(vl, V, (int)ld, C, div_magic((int)ld),
                                                             (aligned16(vl) && ld % 4 == 0) ? 1 : 0, bias, perm,
                                                             vstart, labels, N, lse, kept, partial);
  point_ce_final_kernel<<<1, 256, 0, s>>>(partial, P, loss, n_kept, n_bad);
  return check_launch("msp_voxel_ce_fwd");
}

int msp_voxel_ce_bwd(const float* vl, int64_t V, int64_t ld, int C, const float* bias, const int32_t* perm,
                     const int32_t* vstart, const int64_t* labels, int64_t N, const float* lse, const int32_t* kept,
                     const int64_t* n_kept, const float* gout, const float* gscene, const uint64_t* keys, int shift,
                     int B, const int64_t* npts, float* dvl, msp_stream_t stream) {
  MSP_REQUIRE(C >= 1 && C <= kMaxC, "msp_voxel_ce_bwd: C=%d outside [1, %d]", C, kMaxC);
  MSP_REQUIRE(V >= 0 && N >= 0 && N < (1ll << 31) && ld >= C && ld <= kMaxLd,
              "msp_voxel_ce_bwd: bad arguments (V=%lld N=%lld ld=%lld)", (long long)V, (long long)N, (long long)ld);
  if (V == 0) return MSP_OK;
  MSP_REQUIRE(vl && perm && vstart && labels && lse && kept && n_kept && gout && dvl,
              "msp_voxel_ce_bwd: NULL pointer");
  MSP_REQUIRE(!gscene || (keys && npts && B >= 1 && shift >= 0 && shift < 64),
              "msp_voxel_ce_bwd: the scene term needs keys, npts, B >= 1 and a shift in [0, 64)");
  const int R = tile_rows(C);
  const size_t lds = tile_lds(C) + (size_t)R * (sizeof(float) + sizeof(int));
  voxel_ce_bwd_kernel<<<stream_grid(ceil_div(V, R), lds), R, lds, as_stream(stream)>>>(
      vl, V, (int)ld, C, div_magic((int)ld), (aligned16(vl) && ld % 4 == 0) ? 1 : 0,
      (aligned16(dvl) && ld % 4 == 0) ? 1 : 0, bias, perm, vstart, labels, N, lse, kept, n_kept, gout, gscene, keys,
      shift, B, npts, dvl);
  return check_launch("msp_voxel_ce_bwd");
}

}  // extern "C"
