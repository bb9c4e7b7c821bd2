// Small-tile bf16 MFMA GEMM for MLP-sized products (GemmPParams.variant = 8).
//
// DLRM's MLPs multiply [1024, 512..1024] activations by [512..1024]^2 weights:
// a 256x256-tile kernel puts 16 workgroups on 256 CUs, and the library's
// 64x64 kernels (the Cijk_* MT64x64x64 of profiles/dlrm_kernels_r3.txt) run
// the bias and the activation in separate passes.  Here:
//   * 64 x 64 output tile per workgroup of 4 waves (2 x 2), each wave one
//     32 x 32 v_mfma_f32_32x32x16_bf16 accumulator (C^T: lane = m, registers =
//     4 consecutive n per group, as gemm.hip) -> a 1024 x 1024 output is 256
//     workgroups, one per CU; 32 KB of LDS lets four share a CU;
//   * K-tiles of 64, both operand images 128-byte rows (mfma.h swizzle: row
//     reads and transposed reads conflict free), register-staged double buffer,
//     one barrier per K-tile;
//   * the epilogues fused: bias + activation (+ pre-activation store), and the
//     activation gradient of the producer (result * act'(aux)) with the bias
//     gradient's column sums (wave shuffle reduction, one fp32 atomic per
//     column per wave half), plain alpha / beta (bf16 or fp32 out) and split-K
//     fp32 slabs (reduced by gemmp.hip's splitk_reduce).
// One kernel body holds the tile program (K loop + epilogue); two s_place
// overloads put it to work: the dense one (batched, split-K: bijective XCD remap
// + grouped raster as gemm.hip) and the grouped / ragged one (the expert MLPs of
// a mixture-of-experts block over row ranges kept on the device, moe.hip).  A
// dense product and a one-group grouped product of the same operands are
// therefore bit-identical.
#include <type_traits>

#include "kernels.h"
#include "mfma.h"

namespace ffk {

namespace {

constexpr int SM = 64, SN = 64, SK = 64, SNT = 256;
constexpr int SIMG = SM * SK * 2;  // 8 KiB per operand image
constexpr int SGROUP = 8;

enum SEpi : int { sPlain = 0, sBiasAct = 1, sDact = 2, sSplit = 3 };
// operand layouts, 2 * trans_a + trans_b; the first three are GroupedGemmParams.form
enum SLay : int { sNN = 0, sNT = 1, sTN = 2, sTT = 3 };

// what the tile program reads; s_place points it at the workgroup's product
struct GemmTile {
  const bf16* A;
  const bf16* B;
  void* C;
  const bf16* bias;
  bf16* pre;
  const bf16* aux;
  int M, N, K, lda, ldb, ldc;
  float beta;
  int out_f32;
};

struct GemmSArgs : GemmTile {
  float* ws;
  float* dbias;
  float alpha;
  int splits;
  int64_t sA, sB, sC;   // batched: element strides between the blockIdx.z products
};

// Row blocks [offsets[e], offsets[e+1]) of A / C belong to group e, whose
// weight is B + e * sB.  sNN: C[rows_e] = act(A[rows_e] B[e] + bias[e]); sNT:
// C[rows_e] = A[rows_e] B[e]^T (* act'(aux)); both walk the device-side
// row-tile map of moe_route (tile -> group, first row) and bound the rows by
// the group's end.  sTN: C[e] = beta C[e] + A[rows_e]^T B[rows_e]: the
// contraction runs over the group's rows, rows at and beyond its end enter as
// zeros.
struct GemmGArgs : GemmTile {
  const int* offsets;
  const int* tile_group;
  const int* tile_row0;
  const int* n_tiles;
  int T;
  int64_t sB, sC, sBias;
};

// A workgroup's tile: rows m0 .. m_hi - 1 (at most 64), columns from n0, summed
// over the contraction indices k_lo .. k_hi - 1.
struct STilePos {
  int m0, n0, m_hi, k_lo, k_hi;
};

// s_place<LAY>(g, t): point g at the workgroup's product and t at its tile;
// false: the workgroup has none.  Dense (any LAY):
template <int LAY>
__device__ __forceinline__ bool s_place(GemmSArgs& g, STilePos& t) {
  if (blockIdx.z) {  // batched product z (plain epilogue)
    g.A += blockIdx.z * g.sA;
    g.B += blockIdx.z * g.sB;
    g.C = static_cast<char*>(g.C) + blockIdx.z * g.sC * (g.out_f32 ? 4 : 2);
  }
  const int gm = (g.M + SM - 1) / SM, gn = (g.N + SN - 1) / SN;
  const int nwg = gm * gn;
  const int bid = xcd_remap(blockIdx.x, nwg);
  const int per_group = SGROUP * gn;
  const int first_m = (bid / per_group) * SGROUP;
  const int gsize = min(gm - first_m, SGROUP);
  const int m0 = (first_m + (bid % per_group) % gsize) * SM;
  const int n0 = ((bid % per_group) / gsize) * SN;

  // split-K: split blockIdx.y takes a contiguous (uneven) range of K-tiles
  const int nk_all = g.K / SK;
  const int sb = nk_all / g.splits, sr = nk_all % g.splits, sp = blockIdx.y;
  const int kt0 = sp * sb + min(sp, sr);
  const int kt1 = kt0 + sb + (sp < sr ? 1 : 0);
  t = STilePos{m0, n0, g.M, kt0 * SK, kt1 * SK};
  return true;
}

// Grouped: the row-tile map (sNN, sNT) or one group's rows as the contraction range (sTN)
template <int LAY>
__device__ __forceinline__ bool s_place(GemmGArgs& g, STilePos& t) {
  int e, m0, n0, m_hi, k_lo, k_hi;
  if (LAY == sTN) {
    e = blockIdx.z;
    m0 = blockIdx.x * SM;
    n0 = blockIdx.y * SN;
    m_hi = g.M;
    k_lo = g.offsets[e];
    k_hi = g.offsets[e + 1];
    if (k_hi <= k_lo && g.beta != 0.f) return false;  // empty group, accumulate: C[e] stays
    g.C = static_cast<char*>(g.C) + e * g.sC * (g.out_f32 ? 4 : 2);
  } else {
    const int tile = blockIdx.x % g.T;
    if (tile >= *g.n_tiles) return false;  // the grid is sized by the static tile bound
    e = g.tile_group[tile];
    m0 = g.tile_row0[tile];
    n0 = (blockIdx.x / g.T) * SN;
    m_hi = g.offsets[e + 1];
    k_lo = 0;
    k_hi = g.K;
    g.B += e * g.sB;
    if (g.bias) g.bias += e * g.sBias;
  }
  t = STilePos{m0, n0, m_hi, k_lo, k_hi};
  return true;
}

// Two 16-byte chunks per thread per operand tile.  K-contiguous operand:
// image row = the outer index (m or n), chunk = 8 k; K-outer operand: image
// row = k, chunk = 8 outer.  Both images: 64 rows x 128 B.  Chunks at or beyond
// n_outer enter as zeros; with KB so do chunks at or beyond k_hi (K tails, and
// the ragged row ranges of the grouped kernel).  The dense kernel has whole
// K-tiles (K % 64 == 0) and no KB: its loads carry no k_hi comparison.
template <bool KC, bool KB>
struct SStager {
  bf16x8 reg[2];
  __device__ __forceinline__ void load(const bf16* P, int ld, int outer0, int n_outer, int k0, int k_hi) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = threadIdx.x + SNT * i;
      const int r = c >> 3, ch = c & 7;
      bool ok;
      const bf16* src;
      if (KC) {
        ok = outer0 + r < n_outer && (!KB || k0 + ch * 8 < k_hi);
        src = P + static_cast<int64_t>(outer0 + r) * ld + k0 + ch * 8;
      } else {
        ok = outer0 + ch * 8 < n_outer && (!KB || k0 + r < k_hi);
        src = P + static_cast<int64_t>(k0 + r) * ld + outer0 + ch * 8;
      }
      reg[i] = ok ? *reinterpret_cast<const bf16x8*>(src) : bf16x8{};
    }
  }
  __device__ __forceinline__ void store(unsigned char* img) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = threadIdx.x + SNT * i;
      *reinterpret_cast<bf16x8*>(img + img_off<128>(c >> 3, c & 7)) = reg[i];
    }
  }
};

// The tile program.  Args picks the placement; the dense arguments alone carry
// alpha, the dbias column sums and the split-K slabs, so the grouped kernels
// get none of that code.  K loop and epilogue stand in the kernel itself: moved
// into inline functions, the same statements compile to a longer K loop on more
// registers (NN plain: 84 -> 89 instructions, 81 -> 84 VGPRs).
template <class Args, int LAY, int EPI, int ACT>
__global__ __launch_bounds__(SNT) void gemms_kernel(Args g) {
  constexpr bool DENSE = std::is_same<Args, GemmSArgs>::value;
  constexpr bool AKC = LAY == sNN || LAY == sNT, BKC = LAY == sNT || LAY == sTT;  // operand is K-contiguous
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * SIMG];  // A0 B0 A1 B1
  STilePos t;
  if (!s_place<LAY>(g, t)) return;
  const int m0 = t.m0, n0 = t.n0, m_hi = t.m_hi, k_lo = t.k_lo, k_hi = t.k_hi;
  // K-tiles kt0 .. kt1 - 1 counted from k_base.  Dense: whole tiles of K.  Kept apart per kind: either
  // kind's form (tiles of K, or tiles counted from k_lo) compiles to a different K loop in the other.
  const int k_base = DENSE ? 0 : k_lo, kt0 = DENSE ? k_lo / SK : 0;
  const int kt1 = DENSE ? k_hi / SK : (k_hi - k_lo + SK - 1) / SK;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  SStager<AKC, !DENSE> sa;
  SStager<BKC, !DENSE> sb;
  f32x16 acc = f32x16{};
  sa.load(g.A, g.lda, m0, m_hi, k_base + kt0 * SK, k_hi);
  sb.load(g.B, g.ldb, n0, g.N, k_base + kt0 * SK, k_hi);
  sa.store(smem);
  sb.store(smem + SIMG);
  __syncthreads();
  for (int kt = kt0; kt < kt1; ++kt) {
    const unsigned char* Ai = smem + ((kt - kt0) & 1) * 2 * SIMG;
    const unsigned char* Bi = Ai + SIMG;
    const bool has_next = kt + 1 < kt1;
    if (has_next) {
      sa.load(g.A, g.lda, m0, m_hi, k_base + (kt + 1) * SK, k_hi);
      sb.load(g.B, g.ldb, n0, g.N, k_base + (kt + 1) * SK, k_hi);
    }
#pragma unroll
    for (int ks = 0; ks < SK / 16; ++ks) {
      const bf16x8 af = AKC ? row_frag<128>(Ai, wm * 32, ks * 16, lane) : tr_frag_nat<128>(Ai, ks * 16, wm * 32, lane);
      const bf16x8 bf = BKC ? row_frag<128>(Bi, wn * 32, ks * 16, lane) : tr_frag_nat<128>(Bi, ks * 16, wn * 32, lane);
      acc = mfma32(bf, af, acc);
    }
    if (has_next) {
      unsigned char* nxt = smem + ((kt + 1 - kt0) & 1) * 2 * SIMG;
      sa.store(nxt);
      sb.store(nxt + SIMG);
    }
    __syncthreads();
  }

  // ---- epilogue: lane row m, columns n = 8 g4 + 4 h + e (acc[4 g4 + e])
  const int h = lane >> 5;
  const int m = m0 + wm * 32 + (lane & 31);
  const bool mok = m < m_hi;
  const int64_t roff = static_cast<int64_t>(mok ? m : m_hi - 1) * g.ldc;
  float csum[16];
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const int n = n0 + wn * 32 + 8 * g4 + 4 * h;
    const bool ok = mok && n < g.N;  // N % 8 == 0: a 4-group is all in or all out
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = acc[4 * g4 + e];
    if constexpr (DENSE) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= g.alpha;
      if (EPI == sSplit) {
        const int sp = blockIdx.y;
        if (ok)
          *reinterpret_cast<f32x4*>(g.ws + (static_cast<int64_t>(sp) * g.M + m) * g.N + n) =
              f32x4{v[0], v[1], v[2], v[3]};
        continue;
      }
    }
    if (EPI == sBiasAct) {
      if (g.bias && n < g.N) {
        const bf16x4 bb = *reinterpret_cast<const bf16x4*>(g.bias + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += bf2f(bb[e]);
      }
      if (g.pre && ok) {
        bf16x4 pv;
#pragma unroll
        for (int e = 0; e < 4; ++e) pv[e] = f2bf(v[e]);
        *reinterpret_cast<bf16x4*>(g.pre + roff + n) = pv;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_ct<ACT>(v[e]);
    }
    if (EPI == sDact) {
      bf16x4 xa{};
      if (ok) xa = *reinterpret_cast<const bf16x4*>(g.aux + roff + n);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] *= act_grad_ct<ACT>(bf2f(xa[e]));
        if (DENSE) csum[4 * g4 + e] = ok ? v[e] : 0.f;
      }
    }
    if (!ok) continue;
    if (g.out_f32) {
      float* C = static_cast<float*>(g.C) + roff + n;
      f32x4 o;
      if (EPI == sPlain && g.beta != 0.f) o = *reinterpret_cast<const f32x4*>(C);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = v[e] + ((EPI == sPlain && g.beta != 0.f) ? g.beta * o[e] : 0.f);
      *reinterpret_cast<f32x4*>(C) = o;
    } else {
      bf16* C = static_cast<bf16*>(g.C) + roff + n;
      if (EPI == sPlain && g.beta != 0.f) {
        const bf16x4 old = *reinterpret_cast<const bf16x4*>(C);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += g.beta * bf2f(old[e]);
      }
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
      *reinterpret_cast<bf16x4*>(C) = o;
    }
  }
  if constexpr (DENSE) {
    if (EPI == sDact && g.dbias) {
      // column sums over the 32 rows of each wave half (lanes with equal h)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) csum[i] += __shfl_xor(csum[i], o, 64);
      }
      if ((lane & 31) == 0) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int n = n0 + wn * 32 + 8 * g4 + 4 * h;
          if (n < g.N) {
#pragma unroll
            for (int e = 0; e < 4; ++e) atomicAdd(g.dbias + n + e, csum[4 * g4 + e]);
          }
        }
      }
    }
  }
}

template <int V>
using IC = std::integral_constant<int, V>;

// Run-time (layout, epilogue, activation) -> the kernel instantiation.  The
// plain and split-K epilogues apply no activation and exist for ACT = 0 only;
// of the grouped forms there is no sTT, no split-K, and sTN is plain only
// (grouped_gemm_bf16 has refused those).
template <class Args>
void s_launch(int lay, int epi, int act, dim3 grid, const Args& g, hipStream_t st) {
  auto launch = [&](auto l, auto e, auto a) {
    if constexpr (std::is_same<Args, GemmSArgs>::value ||
                  (l.value != sTT && e.value != sSplit && (l.value != sTN || e.value == sPlain)))
      hipLaunchKernelGGL((gemms_kernel<Args, l.value, e.value, a.value>), grid, dim3(SNT), 0, st, g);
  };
  auto by_act = [&](auto l, auto e) {
    if constexpr (e.value == sPlain || e.value == sSplit) {
      launch(l, e, IC<0>{});
    } else {
      switch (act) {
        case 1: launch(l, e, IC<1>{}); break;
        case 2: launch(l, e, IC<2>{}); break;
        case 3: launch(l, e, IC<3>{}); break;
        case 4: launch(l, e, IC<4>{}); break;
        default: launch(l, e, IC<0>{}); break;
      }
    }
  };
  auto by_epi = [&](auto l) {
    switch (epi) {
      case sBiasAct: by_act(l, IC<sBiasAct>{}); break;
      case sDact: by_act(l, IC<sDact>{}); break;
      case sSplit: by_act(l, IC<sSplit>{}); break;
      default: by_act(l, IC<sPlain>{}); break;
    }
  };
  switch (lay) {
    case sNT: by_epi(IC<sNT>{}); break;
    case sTN: by_epi(IC<sTN>{}); break;
    case sTT: by_epi(IC<sTT>{}); break;
    default: by_epi(IC<sNN>{}); break;
  }
}

// the fields both parameter structs share, by name
template <class P>
GemmTile tile_of(const P& p) {
  return {static_cast<const bf16*>(p.A), static_cast<const bf16*>(p.B), p.C, static_cast<const bf16*>(p.bias),
          static_cast<bf16*>(p.pre), static_cast<const bf16*>(p.aux), p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.beta,
          p.out_f32};
}

}  // namespace

void grouped_gemm_bf16(const GroupedGemmParams& p, hipStream_t st) {
  if (p.El <= 0 || p.N <= 0 || p.K <= 0 || p.T <= 0) return;
  if (p.form < 0 || p.form > 2) throw std::invalid_argument("grouped_gemm: form is 0 (NN), 1 (NT) or 2 (TN)");
  if (p.N % 8 || p.K % 8 || p.lda % 8 || p.ldb % 8 || p.ldc % 8 || p.sB % 8 || p.sC % 4 || p.sBias % 4)
    throw std::invalid_argument("grouped_gemm: N, K, leading dimensions and group strides must be multiples of 8");
  if ((reinterpret_cast<uintptr_t>(p.A) | reinterpret_cast<uintptr_t>(p.B) | reinterpret_cast<uintptr_t>(p.C) |
       reinterpret_cast<uintptr_t>(p.bias) | reinterpret_cast<uintptr_t>(p.pre) | reinterpret_cast<uintptr_t>(p.aux)) & 15)
    throw std::invalid_argument("grouped_gemm: operands must be 16-byte aligned");
  if (!p.offsets || (p.form != sTN && (!p.tile_group || !p.tile_row0 || !p.n_tiles)))
    throw std::invalid_argument("grouped_gemm: missing offsets / tile map");
  const int epi = p.act_bwd ? sDact : (p.bias || p.pre || p.act) ? sBiasAct : sPlain;
  if (p.form == sTN && p.M % 8) throw std::invalid_argument("grouped_gemm: M must be a multiple of 8");
  if (p.form == sTN && epi != sPlain) throw std::invalid_argument("grouped_gemm: the weight-gradient form is plain");
  if (epi != sPlain && (p.beta != 0.f || p.out_f32))
    throw std::invalid_argument("grouped_gemm: the fused epilogues write bf16 without beta");
  if (epi == sDact && (!p.aux || p.bias || p.pre))
    throw std::invalid_argument("grouped_gemm: the activation-gradient epilogue needs aux, no bias / pre");
  if (p.beta != 0.f && p.beta != 1.f) throw std::invalid_argument("grouped_gemm: beta is 0 or 1");
  if (p.act < 0 || p.act > 4) throw std::invalid_argument("grouped_gemm: unsupported activation");
  GemmGArgs g{tile_of(p), p.offsets, p.tile_group, p.tile_row0, p.n_tiles, p.T, p.sB, p.sC, p.sBias};
  const int gn = (p.N + SN - 1) / SN;
  dim3 grid;
  if (p.form == sTN) {
    if (p.M <= 0) return;
    grid = dim3((p.M + SM - 1) / SM, gn, p.El);
    if (grid.y > 65535 || grid.z > 65535) throw std::invalid_argument("grouped_gemm: grid too large");
  } else {
    grid = dim3(static_cast<unsigned>(p.T) * gn);
  }
  s_launch(p.form, epi, p.act, grid, g, st);
  FFK_LAUNCH_CHECK("grouped_gemm");
}

bool gemms_supported(const GemmPParams& p) {
  return p.K % SK == 0 && p.N % 8 == 0 && p.M % 8 == 0 && p.lda % 8 == 0 && p.ldb % 8 == 0;
}

void gemms_launch(const GemmPParams& p, int splits, hipStream_t st) { gemms_launch_batched(p, splits, 1, 0, 0, 0, st); }

void gemms_launch_batched(const GemmPParams& p, int splits, int batch, int64_t sA, int64_t sB, int64_t sC,
                          hipStream_t st) {
  if (!gemms_supported(p)) throw std::invalid_argument("gemms: needs K % 64, M / N / lda / ldb multiples of 8");
  const int epi = splits > 1 ? sSplit : p.act_bwd ? sDact : (p.bias || p.pre || p.act) ? sBiasAct : sPlain;
  if (epi == sBiasAct && (p.beta != 0.f || p.out_f32))
    throw std::invalid_argument("gemms: the bias / activation epilogue writes bf16 without beta");
  if (epi == sDact && (p.beta != 0.f || p.out_f32 || p.bias || p.pre))
    throw std::invalid_argument("gemms: the activation-gradient epilogue writes bf16, no beta / bias / pre");
  if (p.dbias && epi != sDact) throw std::invalid_argument("gemms: dbias needs the activation-gradient epilogue");
  GemmSArgs g{tile_of(p), p.workspace, p.dbias, p.alpha, splits, sA, sB, sC};
  if (batch > 1 && epi != sPlain) throw std::invalid_argument("gemms: batched products take the plain epilogue");
  const int nwg = ((p.M + SM - 1) / SM) * ((p.N + SN - 1) / SN);
  dim3 grid(nwg, splits, std::max(1, batch));
  s_launch(2 * p.trans_a + p.trans_b, epi, p.act, grid, g, st);
  FFK_LAUNCH_CHECK("gemms");
}

void bmm_bf16(const void* A, const void* B, void* C, int batch, int M, int N, int K, int lda, int ldb, int ldc,
              int64_t sA, int64_t sB, int64_t sC, bool trans_a, bool trans_b, float alpha, float beta, int out_f32,
              hipStream_t st) {
  if (batch <= 0 || M <= 0 || N <= 0 || K <= 0) return;
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15 || (sA % 8) || (sB % 8))
    throw std::invalid_argument("bmm: operands and batch strides must be 16-byte aligned");
  if (ldc % 4 || sC % 4 || (reinterpret_cast<uintptr_t>(C) & (out_f32 ? 15 : 7)))
    throw std::invalid_argument("bmm: C alignment");
  GemmPParams p;
  p.A = A, p.B = B, p.C = C;
  p.M = M, p.N = N, p.K = K, p.lda = lda, p.ldb = ldb, p.ldc = ldc;
  p.trans_a = trans_a, p.trans_b = trans_b;
  p.alpha = alpha, p.beta = beta, p.out_f32 = out_f32;
  gemms_launch_batched(p, 1, batch, sA, sB, sC, st);
}

}  // namespace ffk
