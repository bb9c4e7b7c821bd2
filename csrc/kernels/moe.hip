// Device-side routing for the EXPERTS operator (ops/moe.py): everything the
// grouped GEMMs of gemms.hip need is produced on the GPU, with no host sync,
// so a step with a mixture-of-experts block can be captured into a hipGraph.
//
//   moe_route        (token, slot) pairs -> per-expert offsets, the stable
//                    expert-major permutation and its inverse, and the map of
//                    64-row tiles the grouped GEMMs walk.  Three launches:
//                    per-block histograms (integer LDS atomics: counts only),
//                    one block that scans them, and a scatter whose in-block
//                    rank counts the earlier equal keys - positions never
//                    depend on the order of an atomic, so the result is the
//                    one of a stable argsort, every time.
//   moe_gather_rows  sorted copy of the token rows (optionally scaled per pair)
//   moe_combine      per-token gather of its k expert rows (replaces index_add_)
//   moe_dgate        per-pair dot products for the gate gradient
//   moe_segment_colsum  per-expert column sums (the bias gradients), fixed order
// bf16 rows move in 16-byte chunks, sums are fp32, no floating-point atomics.
#include "kernels.h"
#include "common.h"

namespace ffk {

namespace {

constexpr int RNT = 256;  // pairs per routing block == threads per block
constexpr int RMAXE = 256;

__device__ __forceinline__ int local_expert(const int* ids, int64_t p, int64_t P, int e0, int El) {
  if (p >= P) return -1;
  const int v = ids[p] - e0;
  return (v >= 0 && v < El) ? v : -1;
}

__global__ __launch_bounds__(RNT) void route_hist(const int* ids, int64_t P, int e0, int El, int* ws) {
  __shared__ int hist[RMAXE];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int le = local_expert(ids, static_cast<int64_t>(blockIdx.x) * RNT + threadIdx.x, P, e0, El);
  if (le >= 0) atomicAdd(&hist[le], 1);
  __syncthreads();
  if (threadIdx.x < El) ws[static_cast<int64_t>(blockIdx.x) * El + threadIdx.x] = hist[threadIdx.x];
}

// one block: thread e turns expert e's per-block counts into exclusive bases,
// then the offsets and the tile map are laid out
__global__ __launch_bounds__(RNT) void route_scan(int nb, int El, int* ws, int* offsets, int* tile_group,
                                                  int* tile_row0, int* n_tiles, int T) {
  __shared__ int cnt[RMAXE], off[RMAXE + 1], tile0[RMAXE + 1];
  const int e = threadIdx.x;
  int run = 0;
  if (e < El) {
    for (int b = 0; b < nb; ++b) {
      const int64_t i = static_cast<int64_t>(b) * El + e;
      const int c = ws[i];
      ws[i] = run;
      run += c;
    }
  }
  cnt[e] = run;
  __syncthreads();
  if (e == 0) {
    int o = 0, t = 0;
    for (int i = 0; i < El; ++i) {
      off[i] = o;
      tile0[i] = t;
      o += cnt[i];
      t += (cnt[i] + 63) >> 6;
    }
    off[El] = o;
    tile0[El] = t;
  }
  __syncthreads();
  const int n = off[El], nt = tile0[El];
  if (e < El) {
    offsets[e] = off[e];
    const int tiles = (cnt[e] + 63) >> 6;
    for (int i = 0; i < tiles; ++i) {
      const int t = tile0[e] + i;
      if (t < T) {  // always: sum ceil(cnt / 64) <= ceil(P / 64) + El = T
        tile_group[t] = e;
        tile_row0[t] = off[e] + 64 * i;
      }
    }
  }
  if (e == 0) {
    offsets[El] = n;
    *n_tiles = nt < T ? nt : T;
  }
  for (int t = nt + e; t < T; t += RNT) {
    tile_group[t] = -1;
    tile_row0[t] = n;
  }
}

__global__ __launch_bounds__(RNT) void route_scatter(const int* ids, int64_t P, int e0, int El, const int* ws,
                                                     const int* offsets, int* perm, int* pos) {
  __shared__ int keys[RNT];
  const int64_t p = static_cast<int64_t>(blockIdx.x) * RNT + threadIdx.x;
  const int le = local_expert(ids, p, P, e0, El);
  keys[threadIdx.x] = le;
  __syncthreads();
  int rank = 0;  // earlier pairs of this block with the same expert: stable
  for (int j = 0; j < RNT; ++j) rank += (j < static_cast<int>(threadIdx.x) && keys[j] == le) ? 1 : 0;
  if (p >= P) return;
  const int n = offsets[El];
  if (le >= 0) {
    const int q = offsets[le] + ws[static_cast<int64_t>(blockIdx.x) * El + le] + rank;
    perm[q] = static_cast<int>(p);
    pos[p] = q;
  } else {
    pos[p] = -1;
  }
  if (p >= n) perm[p] = 0;  // positions beyond the local pairs: any valid pair
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const bf16* x, const int* perm, const bf16* scale,
                                                          const int* n_ptr, bf16* xs, int64_t P, int Dc, int k) {
  const int n = *n_ptr;
  const int64_t total = P * Dc;
  for (int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; c < total;
       c += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t p = c / Dc;
    const int ch = static_cast<int>(c - p * Dc);
    bf16x8 v{};
    if (p < n) {
      const int pr = perm[p];
      v = *reinterpret_cast<const bf16x8*>(x + (static_cast<int64_t>(pr / k) * Dc + ch) * 8);
      if (scale) {
        const float s = bf2f(scale[pr]);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = f2bf(bf2f(v[i]) * s);
      }
    }
    *reinterpret_cast<bf16x8*>(xs + c * 8) = v;
  }
}

__global__ __launch_bounds__(256) void combine_kernel(const bf16* y, const int* pos, const bf16* gate, bf16* out,
                                                      int64_t B, int k, int Oc) {
  const int64_t total = B * Oc;
  for (int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; c < total;
       c += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t b = c / Oc;
    const int ch = static_cast<int>(c - b * Oc);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
      const int q = pos[b * k + j];
      if (q < 0) continue;
      const float gv = gate ? bf2f(gate[b * k + j]) : 1.f;
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(y + (static_cast<int64_t>(q) * Oc + ch) * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += gv * bf2f(v[i]);
    }
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = f2bf(acc[i]);
    *reinterpret_cast<bf16x8*>(out + c * 8) = o;
  }
}

// one wave per (token, slot) pair
__global__ __launch_bounds__(256) void dgate_kernel(const bf16* dout, const bf16* y, const int* pos, float* dgate,
                                                    int64_t pairs, int k, int Oc) {
  const int lane = threadIdx.x & 63;
  const int64_t pr = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (pr >= pairs) return;
  const int q = pos[pr];
  float acc = 0.f;
  if (q >= 0) {
    const bf16* dr = dout + (pr / k) * Oc * 8;
    const bf16* yr = y + static_cast<int64_t>(q) * Oc * 8;
    for (int ch = lane; ch < Oc; ch += 64) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(dr + ch * 8);
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(yr + ch * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc += bf2f(a[i]) * bf2f(b[i]);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) dgate[pr] = acc;
}

// block = 64 columns x 32 row lanes of one expert's row range
__global__ __launch_bounds__(256) void segment_colsum_kernel(const bf16* x, const int* offsets, float* out, int N) {
  __shared__ float part[32][65];
  const int e = blockIdx.y;
  const int ch = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int col = blockIdx.x * 64 + ch * 8;
  const int lo = offsets[e], hi = offsets[e + 1];
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (col < N) {
    for (int r = lo + rl; r < hi; r += 32) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + static_cast<int64_t>(r) * N + col);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] += bf2f(v[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) part[rl][ch * 8 + i] = acc[i];
  __syncthreads();
  if (threadIdx.x < 64) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 32; ++r) s += part[r][threadIdx.x];
    if (n < N) out[static_cast<int64_t>(e) * N + n] = s;
  }
}

void need16(const void* p, const char* what) {
  if (reinterpret_cast<uintptr_t>(p) & 15) throw std::invalid_argument(std::string(what) + ": 16-byte alignment");
}

}  // namespace

int64_t moe_route_ws(int64_t P, int El) { return ((P + RNT - 1) / RNT) * static_cast<int64_t>(El); }

void moe_route(const int* ids, int64_t P, int e0, int El, int* offsets, int* perm, int* pos, int* tile_group,
               int* tile_row0, int* n_tiles, int T, int* ws, hipStream_t st) {
  if (El < 1 || El > RMAXE) throw std::invalid_argument("moe_route: 1 <= local experts <= 256");
  if (P < 1 || P > (int64_t{1} << 30)) throw std::invalid_argument("moe_route: pair count out of range");
  if (T < (P + 63) / 64 + El) throw std::invalid_argument("moe_route: tile map smaller than ceil(P / 64) + El");
  const int nb = static_cast<int>((P + RNT - 1) / RNT);
  hipLaunchKernelGGL(route_hist, dim3(nb), dim3(RNT), 0, st, ids, P, e0, El, ws);
  hipLaunchKernelGGL(route_scan, dim3(1), dim3(RNT), 0, st, nb, El, ws, offsets, tile_group, tile_row0, n_tiles, T);
  hipLaunchKernelGGL(route_scatter, dim3(nb), dim3(RNT), 0, st, ids, P, e0, El, ws, offsets, perm, pos);
  FFK_LAUNCH_CHECK("moe_route");
}

void moe_gather_rows(const void* x, const int* perm, const void* scale, const int* n_ptr, void* xs, int64_t P,
                     int D, int k, hipStream_t st) {
  if (P <= 0 || D <= 0) return;
  if (D % 8 || k < 1) throw std::invalid_argument("moe_gather_rows: D % 8 == 0, k >= 1");
  need16(x, "moe_gather_rows x");
  need16(xs, "moe_gather_rows xs");
  hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(P * (D / 8), 256)), dim3(256), 0, st,
                     static_cast<const bf16*>(x), perm, static_cast<const bf16*>(scale), n_ptr,
                     static_cast<bf16*>(xs), P, D / 8, k);
  FFK_LAUNCH_CHECK("moe_gather_rows");
}

void moe_combine(const void* y, const int* pos, const void* gate, void* out, int64_t B, int k, int O,
                 hipStream_t st) {
  if (B <= 0 || O <= 0) return;
  if (O % 8 || k < 1) throw std::invalid_argument("moe_combine: O % 8 == 0, k >= 1");
  need16(y, "moe_combine y");
  need16(out, "moe_combine out");
  hipLaunchKernelGGL(combine_kernel, dim3(grid_for(B * (O / 8), 256)), dim3(256), 0, st, static_cast<const bf16*>(y),
                     pos, static_cast<const bf16*>(gate), static_cast<bf16*>(out), B, k, O / 8);
  FFK_LAUNCH_CHECK("moe_combine");
}

void moe_dgate(const void* dout, const void* y, const int* pos, float* dgate, int64_t B, int k, int O,
               hipStream_t st) {
  if (B <= 0 || O <= 0) return;
  if (O % 8 || k < 1) throw std::invalid_argument("moe_dgate: O % 8 == 0, k >= 1");
  need16(dout, "moe_dgate dout");
  need16(y, "moe_dgate y");
  const int64_t pairs = B * k;
  if ((pairs + 3) / 4 > 0x7fffffff) throw std::invalid_argument("moe_dgate: too many pairs");
  hipLaunchKernelGGL(dgate_kernel, dim3(static_cast<unsigned>((pairs + 3) / 4)), dim3(256), 0, st,
                     static_cast<const bf16*>(dout), static_cast<const bf16*>(y), pos, dgate, pairs, k, O / 8);
  FFK_LAUNCH_CHECK("moe_dgate");
}

void moe_segment_colsum(const void* x, const int* offsets, float* out, int El, int N, hipStream_t st) {
  if (El <= 0 || N <= 0) return;
  if (N % 8 || El > 65535) throw std::invalid_argument("moe_segment_colsum: N % 8 == 0, El <= 65535");
  need16(x, "moe_segment_colsum x");
  hipLaunchKernelGGL(segment_colsum_kernel, dim3((N + 63) / 64, El), dim3(256), 0, st, static_cast<const bf16*>(x),
                     offsets, out, N);
  FFK_LAUNCH_CHECK("moe_segment_colsum");
}

}  // namespace ffk
