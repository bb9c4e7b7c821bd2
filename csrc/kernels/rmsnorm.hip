// RMSNorm (optionally fused with the residual add) forward / backward and the
// rotary position embedding for gfx950.  Both are bandwidth bound: 16-byte
// loads / stores, fp32 math, no MFMA.
//
// RMSNorm: y = s * rstd * gamma, rstd = rsqrt(mean(s^2) + eps), s = x (+ res).
// A row of N = C * L * 8 elements is held in the registers of a group of L
// lanes (8 elements per lane per chunk):
//  * N in {64, 128, 256}: L = N / 8 in {8, 16, 32}, 64 / L rows per wave, the
//    reductions stay inside the group (QK-norm rows: no idle lane);
//  * N = C * 512, C <= 8: L = 64, one wave per row;
//  * any other N % 8 == 0: one 256-thread block per row, two passes.
// dgamma is deterministic: every block stores its column partials with plain
// stores into ws[grid][N] and one pass adds each column in a fixed order.
#include "common.h"

#include <algorithm>

#include "kernels.h"

namespace ffk {

namespace {

template <typename T>
struct RVec8;
template <>
struct RVec8<bf16> {
  static __device__ __forceinline__ void load(const bf16* p, float* o) {
    u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = u2f(v[i]);
  }
  static __device__ __forceinline__ void store(bf16* p, const float* o) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = f2bf(o[i]);
    *reinterpret_cast<bf16x8*>(p) = v;
  }
};
template <>
struct RVec8<float> {
  static __device__ __forceinline__ void load(const float* p, float* o) {
    f32x4 a = reinterpret_cast<const f32x4*>(p)[0];
    f32x4 b = reinterpret_cast<const f32x4*>(p)[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = a[i];
      o[4 + i] = b[i];
    }
  }
  static __device__ __forceinline__ void store(float* p, const float* o) {
    f32x4 a, b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = o[i];
      b[i] = o[4 + i];
    }
    reinterpret_cast<f32x4*>(p)[0] = a;
    reinterpret_cast<f32x4*>(p)[1] = b;
  }
};

// sum over the L consecutive lanes that hold one row (L a power of two <= 64)
template <int L>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------
template <typename T, int L, int C>
__global__ __launch_bounds__(256) void rms_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                      T* __restrict__ sum_out, const T* __restrict__ gamma,
                                                      T* __restrict__ y, float* __restrict__ rstd_out, int M,
                                                      float eps) {
  constexpr int N = C * L * 8;
  constexpr int RPB = 256 / L;  // rows per block
  const int l = threadIdx.x % L;
  const int row = blockIdx.x * RPB + threadIdx.x / L;
  if (row >= M) return;  // the whole group leaves: the shuffles below stay inside a group
  const size_t base = static_cast<size_t>(row) * N;
  float v[C][8];
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int col = (c * L + l) * 8;
    RVec8<T>::load(x + base + col, v[c]);
    if (res) {
      float r[8];
      RVec8<T>::load(res + base + col, r);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[c][i] += r[i];
      if (sum_out) RVec8<T>::store(sum_out + base + col, v[c]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) q += v[c][i] * v[c][i];
  }
  const float rstd = rsqrtf(group_sum<L>(q) * (1.f / N) + eps);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int col = (c * L + l) * 8;
    float o[8];
    if (gamma) {
      float g[8];
      RVec8<T>::load(gamma + col, g);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = v[c][i] * rstd * g[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = v[c][i] * rstd;
    }
    RVec8<T>::store(y + base + col, o);
  }
  if (l == 0) rstd_out[row] = rstd;
}

// any N % 8 == 0: one block per row, two passes over the row (L2 resident)
template <typename T>
__global__ __launch_bounds__(256) void rms_fwd_generic(const T* __restrict__ x, const T* __restrict__ res,
                                                       T* __restrict__ sum_out, const T* __restrict__ gamma,
                                                       T* __restrict__ y, float* __restrict__ rstd_out, int N,
                                                       float eps) {
  __shared__ float scratch[4];
  const int row = blockIdx.x;
  const size_t base = static_cast<size_t>(row) * N;
  float q = 0.f;
  for (int col = threadIdx.x * 8; col < N; col += 256 * 8) {
    float v[8];
    RVec8<T>::load(x + base + col, v);
    if (res) {
      float r[8];
      RVec8<T>::load(res + base + col, r);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += r[i];
      if (sum_out) RVec8<T>::store(sum_out + base + col, v);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) q += v[i] * v[i];
  }
  const float rstd = rsqrtf(block_sum<256>(q, scratch) / N + eps);
  for (int col = threadIdx.x * 8; col < N; col += 256 * 8) {
    float v[8], o[8];
    RVec8<T>::load(x + base + col, v);
    if (res) {
      float r[8];
      RVec8<T>::load(res + base + col, r);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += r[i];
    }
    if (gamma) {
      float g[8];
      RVec8<T>::load(gamma + col, g);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = v[i] * rstd * g[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = v[i] * rstd;
    }
    RVec8<T>::store(y + base + col, o);
  }
  if (threadIdx.x == 0) rstd_out[row] = rstd;
}

// ---------------------------------------------------------------------------
// Backward: xhat = s * rstd, g = dy * gamma
//   dx = rstd * (g - xhat * mean(g * xhat)) (+ dres);  dgamma += colsum(dy * xhat)
// A group visits rows blockIdx * RPB + group, + gridDim * RPB, ..., R of them
// in flight (their loads are issued together).  The dgamma partials stay in
// registers over the rows a group visits, are added over the block's groups
// through LDS in a fixed order and stored to ws[blockIdx][N].
template <typename T, int L, int C, int R>
__global__ __launch_bounds__(256) void rms_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ s,
                                                      const float* __restrict__ rstd_in,
                                                      const T* __restrict__ gamma, T* __restrict__ dx,
                                                      float* __restrict__ ws, int M, const T* __restrict__ dres) {
  constexpr int N = C * L * 8;
  constexpr int RPB = 256 / L;
  __shared__ float red[256 * 8];
  const int l = threadIdx.x % L;
  const int grp = threadIdx.x / L;
  float pg[C][8], gm[C][8];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (gamma) RVec8<T>::load(gamma + (c * L + l) * 8, gm[c]);
    else
#pragma unroll
      for (int i = 0; i < 8; ++i) gm[c][i] = 1.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) pg[c][i] = 0.f;
  }
  const int stride = gridDim.x * RPB;
  for (int row0 = blockIdx.x * RPB + grp; row0 < M; row0 += R * stride) {
    float dv[R][C][8], sv[R][C][8], rv[R][C][8];
    float rstd[R];
    bool ok[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      // row0 + k * stride < 2^31: M < 2^31 and the launcher caps stride * R
      const int row = row0 + k * stride;
      ok[k] = row < M;
      const int rr = ok[k] ? row : row0;
      const size_t base = static_cast<size_t>(rr) * N;
      rstd[k] = rstd_in[rr];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int col = (c * L + l) * 8;
        RVec8<T>::load(dy + base + col, dv[k][c]);
        RVec8<T>::load(s + base + col, sv[k][c]);
        if (dres) RVec8<T>::load(dres + base + col, rv[k][c]);
      }
      if (!ok[k])
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int i = 0; i < 8; ++i) dv[k][c][i] = 0.f;
    }
    float sum_gx[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float xh = sv[k][c][i] * rstd[k];
          sv[k][c][i] = xh;  // keep xhat
          a += dv[k][c][i] * gm[c][i] * xh;
          pg[c][i] += dv[k][c][i] * xh;
        }
      sum_gx[k] = group_sum<L>(a) * (1.f / N);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (!ok[k]) continue;
      const size_t base = static_cast<size_t>(row0 + k * stride) * N;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = rstd[k] * (dv[k][c][i] * gm[c][i] - sv[k][c][i] * sum_gx[k]);
        if (dres) {
#pragma unroll
          for (int i = 0; i < 8; ++i) o[i] += rv[k][c][i];
        }
        RVec8<T>::store(dx + base + (c * L + l) * 8, o);
      }
    }
  }
  if (!ws) return;
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int i = 0; i < 8; ++i) red[(grp * L + l) * 8 + i] = pg[c][i];
    __syncthreads();
    for (int j = threadIdx.x; j < L * 8; j += 256) {
      float a = 0.f;
#pragma unroll
      for (int g = 0; g < RPB; ++g) a += red[g * L * 8 + j];
      ws[static_cast<size_t>(blockIdx.x) * N + c * L * 8 + j] = a;
    }
    __syncthreads();
  }
}

// generic dx: one block per row, two passes
template <typename T>
__global__ __launch_bounds__(256) void rms_bwd_generic(const T* __restrict__ dy, const T* __restrict__ s,
                                                       const float* __restrict__ rstd_in,
                                                       const T* __restrict__ gamma, T* __restrict__ dx, int N,
                                                       const T* __restrict__ dres) {
  __shared__ float scratch[4];
  const int row = blockIdx.x;
  const size_t base = static_cast<size_t>(row) * N;
  const float rstd = rstd_in[row];
  float sum_gx = 0.f;
  for (int col = threadIdx.x * 8; col < N; col += 256 * 8) {
    float dv[8], sv[8], gm[8];
    RVec8<T>::load(dy + base + col, dv);
    RVec8<T>::load(s + base + col, sv);
    if (gamma) RVec8<T>::load(gamma + col, gm);
    else
#pragma unroll
      for (int i = 0; i < 8; ++i) gm[i] = 1.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) sum_gx += dv[i] * gm[i] * (sv[i] * rstd);
  }
  sum_gx = block_sum<256>(sum_gx, scratch) / N;
  for (int col = threadIdx.x * 8; col < N; col += 256 * 8) {
    float dv[8], sv[8], gm[8], o[8];
    RVec8<T>::load(dy + base + col, dv);
    RVec8<T>::load(s + base + col, sv);
    if (gamma) RVec8<T>::load(gamma + col, gm);
    else
#pragma unroll
      for (int i = 0; i < 8; ++i) gm[i] = 1.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = rstd * (dv[i] * gm[i] - sv[i] * rstd * sum_gx);
    if (dres) {
      float r[8];
      RVec8<T>::load(dres + base + col, r);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] += r[i];
    }
    RVec8<T>::store(dx + base + col, o);
  }
}

// generic dgamma partials: block (bx, g) adds dy * s * rstd over the rows
// [g * chunk, (g + 1) * chunk) for 256 columns, one column per thread
template <typename T>
__global__ __launch_bounds__(256) void rms_dgamma_generic(const T* __restrict__ dy, const T* __restrict__ s,
                                                          const float* __restrict__ rstd_in,
                                                          float* __restrict__ ws, int M, int N, int chunk) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  const int r0 = blockIdx.y * chunk;
  const int r1 = min(M, r0 + chunk);
  float a = 0.f;
  for (int r = r0; r < r1; ++r) {
    const size_t at = static_cast<size_t>(r) * N + c;
    a += static_cast<float>(dy[at]) * (static_cast<float>(s[at]) * rstd_in[r]);
  }
  ws[static_cast<size_t>(blockIdx.y) * N + c] = a;
}

// out[c] += sum over the rows of ws[rows][N], in one fixed order: 64 columns x
// 4 row groups per block, group ry adds rows ry, ry + 4, ... in sequence, the
// four group sums are added as (0 + 1) + (2 + 3).  One block owns a column:
// plain read-modify-write, no atomics.
__global__ __launch_bounds__(256) void rms_ws_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                            int rows, int N) {
  __shared__ float red[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  float acc = 0.f;
  if (c < N)
    for (int r = ry; r < rows; r += 4) acc += ws[static_cast<size_t>(r) * N + c];
  red[ry][cx] = acc;
  __syncthreads();
  if (ry == 0 && c < N) out[c] += (red[0][cx] + red[1][cx]) + (red[2][cx] + red[3][cx]);
}

constexpr int kGenericParts = 64;  // row chunks of the generic dgamma pass

inline bool group_path(int N) { return N == 64 || N == 128 || N == 256 || (N % 512 == 0 && N <= 4096); }

template <typename T>
void rms_fwd_t(const void* x, const void* res, void* sum_out, const void* gamma, void* y, float* rstd, int M, int N,
               float eps, hipStream_t st) {
  auto X = static_cast<const T*>(x);
  auto R = static_cast<const T*>(res);
  auto S = static_cast<T*>(sum_out);
  auto G = static_cast<const T*>(gamma);
  auto Y = static_cast<T*>(y);
#define FFK_RMS_FWD(l, c)                                                                                         \
  hipLaunchKernelGGL((rms_fwd_kernel<T, l, c>), dim3((M + 256 / l - 1) / (256 / l)), dim3(256), 0, st, X, R, S, G, \
                     Y, rstd, M, eps)
  switch (group_path(N) ? N : 0) {
    case 64: FFK_RMS_FWD(8, 1); break;
    case 128: FFK_RMS_FWD(16, 1); break;
    case 256: FFK_RMS_FWD(32, 1); break;
    case 512: FFK_RMS_FWD(64, 1); break;
    case 1024: FFK_RMS_FWD(64, 2); break;
    case 1536: FFK_RMS_FWD(64, 3); break;
    case 2048: FFK_RMS_FWD(64, 4); break;
    case 2560: FFK_RMS_FWD(64, 5); break;
    case 3072: FFK_RMS_FWD(64, 6); break;
    case 3584: FFK_RMS_FWD(64, 7); break;
    case 4096: FFK_RMS_FWD(64, 8); break;
    default:
      hipLaunchKernelGGL((rms_fwd_generic<T>), dim3(M), dim3(256), 0, st, X, R, S, G, Y, rstd, N, eps);
  }
#undef FFK_RMS_FWD
  FFK_LAUNCH_CHECK("rmsnorm_fwd");
}

template <typename T>
void rms_bwd_t(const void* dy, const void* s, const float* rstd, const void* gamma, void* dx, float* dgamma,
               float* ws, int M, int N, const void* dres, hipStream_t st) {
  auto DY = static_cast<const T*>(dy);
  auto S = static_cast<const T*>(s);
  auto G = static_cast<const T*>(gamma);
  auto DX = static_cast<T*>(dx);
  auto DR = static_cast<const T*>(dres);
  if (dgamma && ws == nullptr) throw std::invalid_argument("rmsnorm_bwd: workspace required for dgamma");
  float* W = dgamma ? ws : nullptr;
  const int grid = rmsnorm_bwd_grid(M, N);
  // two rows in flight while the row pair, gamma and the partials fit the register file
#define FFK_RMS_BWD(l, c)                                                                                       \
  hipLaunchKernelGGL((rms_bwd_kernel<T, l, c, (c <= 4 ? 2 : 1)>), dim3(grid), dim3(256), 0, st, DY, S, rstd, G, DX, \
                     W, M, DR)
  switch (group_path(N) ? N : 0) {
    case 64: FFK_RMS_BWD(8, 1); break;
    case 128: FFK_RMS_BWD(16, 1); break;
    case 256: FFK_RMS_BWD(32, 1); break;
    case 512: FFK_RMS_BWD(64, 1); break;
    case 1024: FFK_RMS_BWD(64, 2); break;
    case 1536: FFK_RMS_BWD(64, 3); break;
    case 2048: FFK_RMS_BWD(64, 4); break;
    case 2560: FFK_RMS_BWD(64, 5); break;
    case 3072: FFK_RMS_BWD(64, 6); break;
    case 3584: FFK_RMS_BWD(64, 7); break;
    case 4096: FFK_RMS_BWD(64, 8); break;
    default: {
      hipLaunchKernelGGL((rms_bwd_generic<T>), dim3(M), dim3(256), 0, st, DY, S, rstd, G, DX, N, DR);
      if (W) {
        const int chunk = (M + grid - 1) / grid;
        hipLaunchKernelGGL((rms_dgamma_generic<T>), dim3((N + 255) / 256, grid), dim3(256), 0, st, DY, S, rstd, W, M,
                           N, chunk);
      }
    }
  }
#undef FFK_RMS_BWD
  FFK_LAUNCH_CHECK("rmsnorm_bwd");
  if (W) {
    hipLaunchKernelGGL(rms_ws_reduce_kernel, dim3((N + 63) / 64), dim3(256), 0, st, W, dgamma, grid, N);
    FFK_LAUNCH_CHECK("rmsnorm_bwd_reduce");
  }
}

// ---------------------------------------------------------------------------
// RoPE: x viewed as [rows, D], position of a row = (row / inner) % S.  A
// thread owns 8 pairs: it loads both 8-element halves (half-split: [8j, 8j+8)
// and D/2 + the same; interleaved: [16j, 16j+16)), rotates in fp32 with the
// table's (cos, sin) of frequencies 8j .. 8j+7 and stores both, so y may be x.
template <typename T, bool INTERLEAVED>
__global__ __launch_bounds__(256) void rope_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                   const float* __restrict__ table, int64_t rows, int S, int inner,
                                                   int D, float sign) {
  const int tpr = D / 16;  // threads per row
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= rows * tpr) return;
  const int64_t row = idx / tpr;
  const int j = static_cast<int>(idx - row * tpr);
  const int pos = static_cast<int>((row / inner) % S);
  const int oa = INTERLEAVED ? 16 * j : 8 * j;
  const int ob = INTERLEAVED ? 16 * j + 8 : D / 2 + 8 * j;
  const T* xr = x + row * D;
  float a[8], b[8], cs[16];
  RVec8<T>::load(xr + oa, a);
  RVec8<T>::load(xr + ob, b);
  const float* t = table + (static_cast<int64_t>(pos) * (D / 2) + 8 * j) * 2;
  RVec8<float>::load(t, cs);
  RVec8<float>::load(t + 8, cs + 8);
  float oa_v[8], ob_v[8];
  if (INTERLEAVED) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float c0 = cs[2 * p], s0 = sign * cs[2 * p + 1];
      oa_v[2 * p] = a[2 * p] * c0 - a[2 * p + 1] * s0;
      oa_v[2 * p + 1] = a[2 * p + 1] * c0 + a[2 * p] * s0;
      const float c1 = cs[8 + 2 * p], s1 = sign * cs[8 + 2 * p + 1];
      ob_v[2 * p] = b[2 * p] * c1 - b[2 * p + 1] * s1;
      ob_v[2 * p + 1] = b[2 * p + 1] * c1 + b[2 * p] * s1;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float c = cs[2 * i], sn = sign * cs[2 * i + 1];
      oa_v[i] = a[i] * c - b[i] * sn;
      ob_v[i] = b[i] * c + a[i] * sn;
    }
  }
  T* yr = y + row * D;
  RVec8<T>::store(yr + oa, oa_v);
  RVec8<T>::store(yr + ob, ob_v);
}

template <typename T>
void rope_t(const void* x, void* y, const float* table, int64_t rows, int S, int inner, int D, bool interleaved,
            bool inverse, hipStream_t st) {
  const int64_t threads = rows * (D / 16);
  const dim3 grid(static_cast<unsigned>((threads + 255) / 256));
  const float sign = inverse ? -1.f : 1.f;
  if (interleaved)
    hipLaunchKernelGGL((rope_kernel<T, true>), grid, dim3(256), 0, st, static_cast<const T*>(x), static_cast<T*>(y),
                       table, rows, S, inner, D, sign);
  else
    hipLaunchKernelGGL((rope_kernel<T, false>), grid, dim3(256), 0, st, static_cast<const T*>(x),
                       static_cast<T*>(y), table, rows, S, inner, D, sign);
  FFK_LAUNCH_CHECK("rope");
}

}  // namespace

void rmsnorm_fwd(int dtype, const void* x, const void* res, void* sum_out, const void* gamma, void* y, float* rstd,
                 int M, int N, float eps, hipStream_t st) {
  if (N <= 0 || N % 8 != 0) throw std::invalid_argument("rmsnorm: N must be a positive multiple of 8");
  if (M <= 0) return;
  if (dtype == kBF16) rms_fwd_t<bf16>(x, res, sum_out, gamma, y, rstd, M, N, eps, st);
  else if (dtype == kF32) rms_fwd_t<float>(x, res, sum_out, gamma, y, rstd, M, N, eps, st);
  else throw std::invalid_argument("rmsnorm: unsupported dtype");
}

int rmsnorm_bwd_grid(int M, int N) {
  if (M <= 0) return 1;
  if (!group_path(N)) return std::min(M, kGenericParts);
  const int L = N >= 512 ? 64 : N / 8;
  const int per_trip = (256 / L) * (N <= 2048 ? 2 : 1);  // rows a block has in flight
  // narrow rows: more blocks (the partials are only N wide)
  const int cap = N <= 256 ? 1024 : 512;
  return std::max(1, std::min((M + per_trip - 1) / per_trip, cap));
}

void rmsnorm_bwd(int dtype, const void* dy, const void* s, const float* rstd, const void* gamma, void* dx,
                 float* dgamma, float* ws, int M, int N, const void* dres, hipStream_t st) {
  if (N <= 0 || N % 8 != 0) throw std::invalid_argument("rmsnorm: N must be a positive multiple of 8");
  if (M <= 0) return;
  // the row loop steps by at most 2 * 1024 * 32 rows in int arithmetic
  if (M > INT32_MAX - (1 << 17)) throw std::invalid_argument("rmsnorm_bwd: too many rows");
  if (dtype == kBF16) rms_bwd_t<bf16>(dy, s, rstd, gamma, dx, dgamma, ws, M, N, dres, st);
  else if (dtype == kF32) rms_bwd_t<float>(dy, s, rstd, gamma, dx, dgamma, ws, M, N, dres, st);
  else throw std::invalid_argument("rmsnorm: unsupported dtype");
}

void rope(int dtype, const void* x, void* y, const float* table, int64_t rows, int S, int inner, int D,
          bool interleaved, bool inverse, hipStream_t st) {
  if (D <= 0 || D % 16 != 0) throw std::invalid_argument("rope: the rotary dim must be a positive multiple of 16");
  if (S <= 0 || inner <= 0 || rows < 0) throw std::invalid_argument("rope: bad shape");
  if (rows == 0) return;
  if (rows * (D / 16) > (static_cast<int64_t>(1) << 31) * 255) throw std::invalid_argument("rope: tensor too large");
  if (dtype == kBF16) rope_t<bf16>(x, y, table, rows, S, inner, D, interleaved, inverse, st);
  else if (dtype == kF32) rope_t<float>(x, y, table, rows, S, inner, D, interleaved, inverse, st);
  else throw std::invalid_argument("rope: unsupported dtype");
}

}  // namespace ffk
