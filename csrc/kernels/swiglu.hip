// SwiGLU for gfx950: y = silu(g) * u with silu(g) = g * s, s = 1 / (1 + exp(-g)).
//
//   * swiglu_fwd / swiglu_bwd: the gated activation and its gradient over
//     [M, N] operands (bf16 or fp32, N % 8 == 0), 8 elements per thread per
//     step in 16-byte loads and stores.  Every tensor has its own row stride,
//     so gate / up and dgate / dup may be the two halves of one [M, 2N] buffer:
//     the backward is then five passes over [M, N] (read dy, g, u; write dg, du)
//     where the sigmoid / multiply / multiply chain makes about sixteen.
//   * gemm_swiglu: one launch computes g = x Wg and u = x Wu (bf16, fp32
//     accumulation), stores both rounded to bf16 for the backward, and stores
//     y = silu(g) * u computed from the fp32 accumulators and rounded once.
//
// gemm_swiglu's structure is gemm.hip's 128x128x64 register-staged tile with
// the B image shared between the two weights: the workgroup's B image (64 k
// rows x 256 bytes) holds 64 columns of Wg in chunks 0..7 and the SAME 64
// columns of Wu in chunks 8..15, so a workgroup produces a 128 (m) x 64 (n)
// tile of all three outputs.  The 4 waves sit 2 x 2: wave (wm, wn) owns rows
// wm * 64 .. + 64 and the gate block of columns wn * 32 .. + 32 together with
// the matching up block (image columns 64 + wn * 32): 2 x 2 accumulators of
// v_mfma_f32_32x32x16_bf16, each A fragment read from LDS once per k-step and
// fed to both products, each B fragment fed to both row tiles (4 LDS fragment
// reads per 4 MFMAs, as gemm.hip).  Products are computed as C^T, so lane =
// m and a register group = 4 consecutive n: the gate and the up accumulator of
// an output element (m, n) are the same register index of the same lane, and
// the epilogue is straight-line per-lane code with 8-byte stores -- no LDS
// exchange, no shuffle.  Swizzled images (mfma.h), double buffer with the next
// tile's loads issued before the MFMAs and written after them, one barrier per
// K-tile, bijective XCD remap + grouped raster: as gemm.hip.
#include "kernels.h"
#include "mfma.h"
#include "swiglu_math.h"   // swiglu_sigmoid / swiglu_y / swiglu_grad

namespace ffk {

namespace {

// 8 consecutive elements as fp32: one 16-byte access for bf16, two for fp32
template <class T>
__device__ __forceinline__ void load8(const T* p, float (&v)[8]);
template <>
__device__ __forceinline__ void load8<bf16>(const bf16* p, float (&v)[8]) {
  const bf16x8 r = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = bf2f(r[i]);
}
template <>
__device__ __forceinline__ void load8<float>(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = a[i], v[4 + i] = b[i];
}
template <class T>
__device__ __forceinline__ void store8(T* p, const float (&v)[8]);
template <>
__device__ __forceinline__ void store8<bf16>(bf16* p, const float (&v)[8]) {
  bf16x8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = f2bf(v[i]);
  *reinterpret_cast<bf16x8*>(p) = r;
}
template <>
__device__ __forceinline__ void store8<float>(float* p, const float (&v)[8]) {
  *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}

constexpr int ENT = 256;

// chunk c of 8 elements: row c / n8, columns 8 (c % n8) ..
template <class T>
__global__ __launch_bounds__(ENT) void swiglu_fwd_kernel(const T* __restrict__ gate, const T* __restrict__ up,
                                                         T* __restrict__ y, int64_t chunks, int n8, int64_t ldg,
                                                         int64_t ldu, int64_t ldy) {
  for (int64_t c = static_cast<int64_t>(blockIdx.x) * ENT + threadIdx.x; c < chunks;
       c += static_cast<int64_t>(gridDim.x) * ENT) {
    const int64_t m = c / n8;
    const int n = static_cast<int>(c - m * n8) * 8;
    float g[8], u[8], o[8];
    load8(gate + m * ldg + n, g);
    load8(up + m * ldu + n, u);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = swiglu_y(g[i], u[i]);
    store8(y + m * ldy + n, o);
  }
}

// dgate / dup may alias nothing that is read here except through distinct
// columns of one buffer (the halves of [M, 2N]); no __restrict__ on them
template <class T>
__global__ __launch_bounds__(ENT) void swiglu_bwd_kernel(const T* dy, const T* gate, const T* up, T* dgate, T* dup,
                                                         int64_t chunks, int n8, int64_t lddy, int64_t ldg,
                                                         int64_t ldu, int64_t lddg, int64_t lddu) {
  for (int64_t c = static_cast<int64_t>(blockIdx.x) * ENT + threadIdx.x; c < chunks;
       c += static_cast<int64_t>(gridDim.x) * ENT) {
    const int64_t m = c / n8;
    const int n = static_cast<int>(c - m * n8) * 8;
    float d[8], g[8], u[8], dg[8], du[8];
    load8(dy + m * lddy + n, d);
    load8(gate + m * ldg + n, g);
    load8(up + m * ldu + n, u);
#pragma unroll
    for (int i = 0; i < 8; ++i) swiglu_grad(d[i], g[i], u[i], dg[i], du[i]);
    store8(dgate + m * lddg + n, dg);
    store8(dup + m * lddu + n, du);
  }
}

// ---------------------------------------------------------------------------
constexpr int GM = 128, GH = 64, GK = 64;   // rows, columns of EACH weight, k per tile
constexpr int GIMG = GM * GK * 2;           // 16 KiB: A is 128 x 128 B, B is 64 x 256 B
constexpr int GGROUP = 8;

struct SwigluGemmArgs {
  const bf16* X;
  const bf16* Wg;
  const bf16* Wu;
  bf16* G;
  bf16* U;
  bf16* Y;
  int M, N, K, lda, ldb, ldg, ldu, ldy;
};

// A tile: 128 rows (m) x 8 chunks of 8 k, 4 chunks per thread.  Rows at or
// beyond M and chunks at or beyond K (K % 8 == 0: whole chunks) enter as zeros.
struct XStager {
  bf16x8 reg[4];
  __device__ __forceinline__ void load(const bf16* X, int lda, int m0, int M, int k0, int K) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = threadIdx.x + 256 * i;
      const int r = c >> 3, ch = c & 7;
      const bool ok = m0 + r < M && k0 + ch * 8 < K;
      reg[i] = ok ? *reinterpret_cast<const bf16x8*>(X + static_cast<int64_t>(m0 + r) * lda + k0 + ch * 8) : bf16x8{};
    }
  }
  __device__ __forceinline__ void store(unsigned char* img) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = threadIdx.x + 256 * i;
      *reinterpret_cast<bf16x8*>(img + img_off<128>(c >> 3, c & 7)) = reg[i];
    }
  }
};

// B tile: 64 rows (k) x 16 chunks of 8 columns; chunks 0..7 are columns n0 ..
// n0 + 63 of Wg, chunks 8..15 the same columns of Wu.  Rows at or beyond K and
// chunks at or beyond N (N % 8 == 0) enter as zeros.
struct WStager {
  bf16x8 reg[4];
  __device__ __forceinline__ void load(const bf16* Wg, const bf16* Wu, int ldb, int n0, int N, int k0, int K) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = threadIdx.x + 256 * i;
      const int r = c >> 4, ch = c & 15;
      const int n = n0 + (ch & 7) * 8;
      const bool ok = k0 + r < K && n < N;
      const bf16* W = ch < 8 ? Wg : Wu;
      reg[i] = ok ? *reinterpret_cast<const bf16x8*>(W + static_cast<int64_t>(k0 + r) * ldb + n) : bf16x8{};
    }
  }
  __device__ __forceinline__ void store(unsigned char* img) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = threadIdx.x + 256 * i;
      *reinterpret_cast<bf16x8*>(img + img_off<256>(c >> 4, c & 15)) = reg[i];
    }
  }
};

__global__ __launch_bounds__(256, 2) void gemm_swiglu_kernel(SwigluGemmArgs g) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * GIMG];  // A0 B0 A1 B1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave & 1, wn = wave >> 1;

  // ---- tile order: XCD remap, then GGROUP-grouped raster
  const int gm = (g.M + GM - 1) / GM, gn = (g.N + GH - 1) / GH;
  const int nwg = gm * gn;
  const int bid = xcd_remap(blockIdx.x, nwg);
  const int per_group = GGROUP * gn;
  const int first_m = (bid / per_group) * GGROUP;
  const int gsize = min(gm - first_m, GGROUP);
  const int m0 = (first_m + (bid % per_group) % gsize) * GM;
  const int n0 = ((bid % per_group) / gsize) * GH;

  XStager sa;
  WStager sb;
  f32x16 accg[2], accu[2];   // [row tile]: gate and up, same lane, same register index per (m, n)
#pragma unroll
  for (int i = 0; i < 2; ++i) accg[i] = f32x16{}, accu[i] = f32x16{};

  const int nk = (g.K + GK - 1) / GK;
  sa.load(g.X, g.lda, m0, g.M, 0, g.K);
  sb.load(g.Wg, g.Wu, g.ldb, n0, g.N, 0, g.K);
  sa.store(smem);
  sb.store(smem + GIMG);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const unsigned char* Ai = smem + (kt & 1) * 2 * GIMG;
    const unsigned char* Bi = Ai + GIMG;
    const bool has_next = kt + 1 < nk;
    if (has_next) {
      sa.load(g.X, g.lda, m0, g.M, (kt + 1) * GK, g.K);
      sb.load(g.Wg, g.Wu, g.ldb, n0, g.N, (kt + 1) * GK, g.K);
    }
#pragma unroll
    for (int ks = 0; ks < GK / 16; ++ks) {
      const bf16x8 bg = tr_frag_nat<256>(Bi, ks * 16, wn * 32, lane);
      const bf16x8 bu = tr_frag_nat<256>(Bi, ks * 16, GH + wn * 32, lane);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const bf16x8 af = row_frag<128>(Ai, wm * 64 + mt * 32, ks * 16, lane);   // one read, both products
        accg[mt] = mfma32(bg, af, accg[mt]);
        accu[mt] = mfma32(bu, af, accu[mt]);
      }
    }
    if (has_next) {
      unsigned char* nxt = smem + ((kt + 1) & 1) * 2 * GIMG;
      sa.store(nxt);
      sb.store(nxt + GIMG);
    }
    __syncthreads();
  }

  // ---- epilogue: lane row m, columns n = 8 g4 + 4 h + e (acc[4 g4 + e])
  const int h = lane >> 5;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int m = m0 + wm * 64 + mt * 32 + (lane & 31);
    if (m >= g.M) continue;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int n = n0 + wn * 32 + 8 * g4 + 4 * h;
      if (n >= g.N) continue;  // N % 8 == 0: a 4-group is all in or all out
      bf16x4 og, ou, oy;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gv = accg[mt][4 * g4 + e], uv = accu[mt][4 * g4 + e];
        og[e] = f2bf(gv);
        ou[e] = f2bf(uv);
        oy[e] = f2bf(swiglu_y(gv, uv));
      }
      *reinterpret_cast<bf16x4*>(g.G + static_cast<int64_t>(m) * g.ldg + n) = og;
      *reinterpret_cast<bf16x4*>(g.U + static_cast<int64_t>(m) * g.ldu + n) = ou;
      *reinterpret_cast<bf16x4*>(g.Y + static_cast<int64_t>(m) * g.ldy + n) = oy;
    }
  }
}

bool misaligned(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 15) != 0;
}

void check_ew(const char* who, int dtype, int64_t M, int64_t N, std::initializer_list<int64_t> lds,
              std::initializer_list<const void*> ps) {
  const std::string w(who);
  if (dtype != kF32 && dtype != kBF16) throw std::invalid_argument(w + ": operands are bf16 or fp32");
  if (N % 8) throw std::invalid_argument(w + ": N must be a multiple of 8");
  for (int64_t ld : lds)
    if (ld % 8 || ld < N) throw std::invalid_argument(w + ": row strides must be multiples of 8 and at least N");
  for (const void* p : ps)
    if (!p) throw std::invalid_argument(w + ": missing operand");
  if (misaligned(ps)) throw std::invalid_argument(w + ": operands must be 16-byte aligned");
  if (M >= (int64_t(1) << 31) || N >= (int64_t(1) << 31)) throw std::invalid_argument(w + ": M and N must fit 31 bits");
}

}  // namespace

void swiglu_fwd(int dtype, const void* gate, const void* up, void* y, int64_t M, int64_t N, int64_t ldg, int64_t ldu,
                int64_t ldy, hipStream_t st) {
  if (M <= 0 || N <= 0) return;
  check_ew("swiglu_fwd", dtype, M, N, {ldg, ldu, ldy}, {gate, up, y});
  const int64_t chunks = M * (N / 8);
  const dim3 grid(grid_for(chunks, ENT));
  const int n8 = static_cast<int>(N / 8);
  if (dtype == kBF16)
    hipLaunchKernelGGL(swiglu_fwd_kernel<bf16>, grid, dim3(ENT), 0, st, static_cast<const bf16*>(gate),
                       static_cast<const bf16*>(up), static_cast<bf16*>(y), chunks, n8, ldg, ldu, ldy);
  else
    hipLaunchKernelGGL(swiglu_fwd_kernel<float>, grid, dim3(ENT), 0, st, static_cast<const float*>(gate),
                       static_cast<const float*>(up), static_cast<float*>(y), chunks, n8, ldg, ldu, ldy);
  FFK_LAUNCH_CHECK("swiglu_fwd");
}

void swiglu_bwd(int dtype, const void* dy, const void* gate, const void* up, void* dgate, void* dup, int64_t M,
                int64_t N, int64_t lddy, int64_t ldg, int64_t ldu, int64_t lddg, int64_t lddu, hipStream_t st) {
  if (M <= 0 || N <= 0) return;
  check_ew("swiglu_bwd", dtype, M, N, {lddy, ldg, ldu, lddg, lddu}, {dy, gate, up, dgate, dup});
  const int64_t chunks = M * (N / 8);
  const dim3 grid(grid_for(chunks, ENT));
  const int n8 = static_cast<int>(N / 8);
  if (dtype == kBF16)
    hipLaunchKernelGGL(swiglu_bwd_kernel<bf16>, grid, dim3(ENT), 0, st, static_cast<const bf16*>(dy),
                       static_cast<const bf16*>(gate), static_cast<const bf16*>(up), static_cast<bf16*>(dgate),
                       static_cast<bf16*>(dup), chunks, n8, lddy, ldg, ldu, lddg, lddu);
  else
    hipLaunchKernelGGL(swiglu_bwd_kernel<float>, grid, dim3(ENT), 0, st, static_cast<const float*>(dy),
                       static_cast<const float*>(gate), static_cast<const float*>(up), static_cast<float*>(dgate),
                       static_cast<float*>(dup), chunks, n8, lddy, ldg, ldu, lddg, lddu);
  FFK_LAUNCH_CHECK("swiglu_bwd");
}

void gemm_swiglu(const void* x, const void* wg, const void* wu, void* gate_out, void* up_out, void* y, int M, int N,
                 int K, int lda, int ldb, int ldg, int ldu, int ldy, hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0) return;
  if (N % 8 || K % 8) throw std::invalid_argument("gemm_swiglu: N and K must be multiples of 8");
  if (lda % 8 || ldb % 8 || ldg % 8 || ldu % 8 || ldy % 8)
    throw std::invalid_argument("gemm_swiglu: lda, ldb and the output row strides must be multiples of 8");
  if (lda < K || ldb < N || ldg < N || ldu < N || ldy < N)
    throw std::invalid_argument("gemm_swiglu: a row stride is shorter than its row");
  if (!x || !wg || !wu || !gate_out || !up_out || !y) throw std::invalid_argument("gemm_swiglu: missing operand");
  if (misaligned({x, wg, wu, gate_out, up_out, y}))
    throw std::invalid_argument("gemm_swiglu: operands must be 16-byte aligned");
  const int64_t nwg = static_cast<int64_t>((M + GM - 1) / GM) * ((N + GH - 1) / GH);
  if (nwg >= (int64_t(1) << 31)) throw std::invalid_argument("gemm_swiglu: grid too large");
  SwigluGemmArgs g{static_cast<const bf16*>(x), static_cast<const bf16*>(wg), static_cast<const bf16*>(wu),
                   static_cast<bf16*>(gate_out), static_cast<bf16*>(up_out), static_cast<bf16*>(y),
                   M, N, K, lda, ldb, ldg, ldu, ldy};
  hipLaunchKernelGGL(gemm_swiglu_kernel, dim3(static_cast<unsigned>(nwg)), dim3(256), 0, st, g);
  FFK_LAUNCH_CHECK("gemm_swiglu");
}

}  // namespace ffk
