// Gated (SwiGLU) experts for the EXPERTS operator on gfx950: the two grouped
// kernels that ops/moe.py needs beside the grouped products of gemms.hip.
//
//   out[b] = sum_j gate[b, j] * (h W2[e]),  h = silu(g) * u,  [g | u] = x[b] W1[e]
//
// W1 is ONE tensor [El, D, 2H] (columns 0 .. H-1 gate, H .. 2H-1 up), so both
// weight gradients are one grouped TN product with N = 2H and the input
// gradient one grouped NT product with K = 2H (gemms.hip, unchanged).  New:
//
//   A  grouped_gemm_swiglu: over the ragged expert row blocks of moe_route, one
//      launch stores g and u (bf16, the halves of GU [P, 2H]) and h = silu(g) * u
//      computed from the fp32 accumulators and rounded once ([P, H]).
//   B  grouped_gemm_swiglu_bwd: dh = dy[rows_e] W2[e]^T (contraction over O) is
//      never stored; the epilogue reads g, u at the accumulator's own (row,
//      column) and writes dg | du into the halves of DGU [P, 2H].
//
// Geometry of A (the dense ancestor, gemm_swiglu_kernel, has 128-row tiles;
// moe_route's map is in 64-row tiles and an expert's block ends anywhere): a
// workgroup of 4 waves (2 x 2) owns 64 rows x 64 output columns and holds TWO
// 64 x 64 accumulator sets; wave (wm, wn) holds the 32 x 32 gate block and the
// matching up block as C^T (lane = m, register group = 4 consecutive n, as
// gemm.hip), so gate and up of an element are the same register of the same
// lane: the epilogue is per-lane code with 8-byte stores, no LDS exchange, no
// shuffle.  K-tiles of 64: the A image is 64 rows x 128 B (8 KiB), the B image
// 64 k x 256 B (16 KiB: chunks 0..7 = 64 gate columns, chunks 8..15 = the SAME
// 64 columns of the up half), both with the mfma.h swizzle; register-staged
// double buffer (48 KiB, three workgroups per CU), one barrier per K-tile, and
// every A fragment read from LDS feeds both MFMA products (3 fragment reads
// per 2 MFMAs where two 64x64 products would make 4).
//
// B is the 64 x 64 NT tile program of gemms.hip (one accumulator per wave,
// both operands K-contiguous, 32 KiB) with the gated epilogue, which goes
// through LDS to read g, u and write dg, du in whole 16-byte row chunks (see
// the kernel).  It stands here
// as a sibling and not as a further epilogue of gemms_kernel: that leaves the
// existing instantiations' code objects what was measured, and this file is
// compiled without packed fp32 arithmetic (tools/build_native.py).
//
// Placement is the grouped one of gemms.hip: tile t -> (tile_group[t],
// tile_row0[t]), rows bounded by offsets[e + 1], workgroups at or past *n_tiles
// exit.  Rows at or beyond a group's end, and so rows at or beyond offsets[El],
// are never written.  K tails and column tails enter as zeros.
#include "kernels.h"
#include "mfma.h"
#include "swiglu_math.h"

namespace ffk {

namespace {

constexpr int QM = 64, QN = 64, QK = 64, QNT = 256;
constexpr int QIMG = QM * QK * 2;   // 8 KiB: 64 rows x 128 B
constexpr int QIMGW = QK * 256;     // 16 KiB: 64 k x (64 gate | 64 up columns)
constexpr int QPITCH = QN + 4;      // fp32 words per row of kernel B's epilogue tile (17 KiB of its 32)
static_assert(QM * QPITCH * 4 <= 4 * QIMG, "kernel B's epilogue tile must fit its operand images");

struct MoeSwigluArgs {
  const bf16* A;      // A: xs [P, D]           B: dy [P, O]
  const bf16* W;      // A: W1 [El, D, 2H]      B: W2 [El, H, O]
  const bf16* GU;     // B: saved [P, 2H]
  bf16* OUT2;         // A: GU [P, 2H]          B: DGU [P, 2H]
  bf16* Hout;         // A: h [P, H]
  const int* offsets;
  const int* tile_group;
  const int* tile_row0;
  const int* n_tiles;
  int T, K, H;        // K: the contraction length (A: D, B: O)
};

// the workgroup's expert, rows m0 .. m_hi - 1 and first column; false: no tile
__device__ __forceinline__ bool q_place(const MoeSwigluArgs& g, int& e, int& m0, int& m_hi, int& n0) {
  const int tile = blockIdx.x % g.T;
  if (tile >= *g.n_tiles) return false;  // the grid is sized by the static tile bound
  e = g.tile_group[tile];
  m0 = g.tile_row0[tile];
  m_hi = g.offsets[e + 1];
  n0 = (blockIdx.x / g.T) * QN;
  return true;
}

// K-contiguous operand tile: 64 rows (outer index) x 8 chunks of 8 k, two
// chunks per thread.  Rows at or beyond n_outer and chunks at or beyond K
// (K % 8 == 0: whole chunks) enter as zeros.
struct RowStager {
  bf16x8 reg[2];
  __device__ __forceinline__ void load(const bf16* P, int ld, int outer0, int n_outer, int k0, int K) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = threadIdx.x + QNT * i;
      const int r = c >> 3, ch = c & 7;
      const bool ok = outer0 + r < n_outer && k0 + ch * 8 < K;
      reg[i] = ok ? *reinterpret_cast<const bf16x8*>(P + static_cast<int64_t>(outer0 + r) * ld + k0 + ch * 8) : bf16x8{};
    }
  }
  __device__ __forceinline__ void store(unsigned char* img) const {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = threadIdx.x + QNT * i;
      *reinterpret_cast<bf16x8*>(img + img_off<128>(c >> 3, c & 7)) = reg[i];
    }
  }
};

// Dual-weight tile of one fused W1[e] [D, 2H]: 64 rows (k) x 16 chunks of 8
// columns, four chunks per thread; chunks 0..7 are columns n0 .. n0 + 63,
// chunks 8..15 the columns H + n0 .. of the same rows.  Rows at or beyond K and
// chunks at or beyond H (H % 8 == 0) enter as zeros.
struct DualStager {
  bf16x8 reg[4];
  __device__ __forceinline__ void load(const bf16* W, int H, int n0, int k0, int K) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = threadIdx.x + QNT * i;
      const int r = c >> 4, ch = c & 15;
      const int n = n0 + (ch & 7) * 8;
      const bool ok = k0 + r < K && n < H;
      reg[i] = ok ? *reinterpret_cast<const bf16x8*>(W + static_cast<int64_t>(k0 + r) * (2 * H) + (ch < 8 ? 0 : H) + n)
                  : bf16x8{};
    }
  }
  __device__ __forceinline__ void store(unsigned char* img) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = threadIdx.x + QNT * i;
      *reinterpret_cast<bf16x8*>(img + img_off<256>(c >> 4, c & 15)) = reg[i];
    }
  }
};

// ---- kernel A
__global__ __launch_bounds__(QNT) void grouped_gemm_swiglu_kernel(MoeSwigluArgs g) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (QIMG + QIMGW)];  // A0 B0 A1 B1
  int e, m0, m_hi, n0;
  if (!q_place(g, e, m0, m_hi, n0)) return;
  const bf16* W = g.W + static_cast<int64_t>(e) * g.K * (2 * g.H);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave & 1, wn = wave >> 1;

  RowStager sa;
  DualStager sb;
  f32x16 accg = f32x16{}, accu = f32x16{};   // gate and up: same lane, same register index per (m, n)
  const int nk = (g.K + QK - 1) / QK;
  sa.load(g.A, g.K, m0, m_hi, 0, g.K);
  sb.load(W, g.H, n0, 0, g.K);
  sa.store(smem);
  sb.store(smem + QIMG);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const unsigned char* Ai = smem + (kt & 1) * (QIMG + QIMGW);
    const unsigned char* Bi = Ai + QIMG;
    const bool has_next = kt + 1 < nk;
    if (has_next) {
      sa.load(g.A, g.K, m0, m_hi, (kt + 1) * QK, g.K);
      sb.load(W, g.H, n0, (kt + 1) * QK, g.K);
    }
#pragma unroll
    for (int ks = 0; ks < QK / 16; ++ks) {
      const bf16x8 af = row_frag<128>(Ai, wm * 32, ks * 16, lane);   // one read, both products
      const bf16x8 bg = tr_frag_nat<256>(Bi, ks * 16, wn * 32, lane);
      const bf16x8 bu = tr_frag_nat<256>(Bi, ks * 16, QN + wn * 32, lane);
      accg = mfma32(bg, af, accg);
      accu = mfma32(bu, af, accu);
    }
    if (has_next) {
      unsigned char* nxt = smem + ((kt + 1) & 1) * (QIMG + QIMGW);
      sa.store(nxt);
      sb.store(nxt + QIMG);
    }
    __syncthreads();
  }

  // ---- epilogue: lane row m, columns n = 8 g4 + 4 h + i (acc[4 g4 + i])
  const int h = lane >> 5;
  const int m = m0 + wm * 32 + (lane & 31);
  if (m >= m_hi) return;
  bf16* gu = g.OUT2 + static_cast<int64_t>(m) * (2 * g.H);
  bf16* hy = g.Hout + static_cast<int64_t>(m) * g.H;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const int n = n0 + wn * 32 + 8 * g4 + 4 * h;
    if (n >= g.H) continue;  // H % 8 == 0: a 4-group is all in or all out
    bf16x4 og, ou, oy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float gv = accg[4 * g4 + i], uv = accu[4 * g4 + i];
      og[i] = f2bf(gv);
      ou[i] = f2bf(uv);
      oy[i] = f2bf(swiglu_y(gv, uv));
    }
    *reinterpret_cast<bf16x4*>(gu + n) = og;
    *reinterpret_cast<bf16x4*>(gu + g.H + n) = ou;
    *reinterpret_cast<bf16x4*>(hy + n) = oy;
  }
}

// ---- kernel B: dh = dy[rows_e] W2[e]^T, both operands K-contiguous (K = O)
__global__ __launch_bounds__(QNT) void grouped_gemm_swiglu_bwd_kernel(MoeSwigluArgs g) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * QIMG];  // A0 B0 A1 B1
  int e, m0, m_hi, n0;
  if (!q_place(g, e, m0, m_hi, n0)) return;
  const bf16* W = g.W + static_cast<int64_t>(e) * g.H * g.K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave & 1, wn = wave >> 1;

  RowStager sa, sb;
  f32x16 acc = f32x16{};
  const int nk = (g.K + QK - 1) / QK;
  sa.load(g.A, g.K, m0, m_hi, 0, g.K);
  sb.load(W, g.K, n0, g.H, 0, g.K);
  sa.store(smem);
  sb.store(smem + QIMG);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const unsigned char* Ai = smem + (kt & 1) * 2 * QIMG;
    const unsigned char* Bi = Ai + QIMG;
    const bool has_next = kt + 1 < nk;
    if (has_next) {
      sa.load(g.A, g.K, m0, m_hi, (kt + 1) * QK, g.K);
      sb.load(W, g.K, n0, g.H, (kt + 1) * QK, g.K);
    }
#pragma unroll
    for (int ks = 0; ks < QK / 16; ++ks) {
      const bf16x8 af = row_frag<128>(Ai, wm * 32, ks * 16, lane);
      const bf16x8 bf = row_frag<128>(Bi, wn * 32, ks * 16, lane);
      acc = mfma32(bf, af, acc);
    }
    if (has_next) {
      unsigned char* nxt = smem + ((kt + 1) & 1) * 2 * QIMG;
      sa.store(nxt);
      sb.store(nxt + QIMG);
    }
    __syncthreads();
  }

  // ---- gated epilogue: g, u of the accumulator's own (m, n) in, dg | du out.
  // In the C^T orientation a lane owns a row, so reading g, u and writing dg,
  // du from the accumulators is four 8-byte accesses per lane with a row
  // stride between lanes; measured, that cost more than the dh pass it saves
  // (profiles/moe_swiglu.txt).  So dh goes through LDS (free after the K
  // loop's last barrier) as a 64 x 64 fp32 tile, pitch 68 words (16-byte
  // aligned rows, 16 lanes of a 16-byte write on distinct banks), and comes
  // back row-wise: a thread takes 8 consecutive columns of a row, 8 threads a
  // row, every global access 16 bytes and 128 contiguous bytes per row.
  float* dh = reinterpret_cast<float*>(smem);
  const int h = lane >> 5;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4)
    *reinterpret_cast<f32x4*>(dh + (wm * 32 + (lane & 31)) * QPITCH + wn * 32 + 8 * g4 + 4 * h) =
        f32x4{acc[4 * g4], acc[4 * g4 + 1], acc[4 * g4 + 2], acc[4 * g4 + 3]};
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = threadIdx.x + QNT * i;
    const int r = c >> 3, n = n0 + (c & 7) * 8, m = m0 + r;
    if (m >= m_hi || n >= g.H) continue;  // H % 8 == 0: a chunk is all in or all out
    const int64_t off = static_cast<int64_t>(m) * (2 * g.H) + n;
    const bf16x8 gv = *reinterpret_cast<const bf16x8*>(g.GU + off);
    const bf16x8 uv = *reinterpret_cast<const bf16x8*>(g.GU + off + g.H);
    const float* d = dh + r * QPITCH + (c & 7) * 8;
    bf16x8 og, ou;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float dg, du;
      swiglu_grad(d[j], bf2f(gv[j]), bf2f(uv[j]), dg, du);
      og[j] = f2bf(dg);
      ou[j] = f2bf(du);
    }
    *reinterpret_cast<bf16x8*>(g.OUT2 + off) = og;
    *reinterpret_cast<bf16x8*>(g.OUT2 + off + g.H) = ou;
  }
}

// the contract both launches share; returns the grid size
unsigned check_grouped(const char* who, std::initializer_list<const void*> ps, const int* offsets,
                       const int* tile_group, const int* tile_row0, const int* n_tiles, int El, int T, int K, int H) {
  const std::string w(who);
  if (El < 1 || El > MOE_MAX_LOCAL_EXPERTS)
    throw std::invalid_argument(w + ": 1 <= local experts <= " + std::to_string(MOE_MAX_LOCAL_EXPERTS));
  if (K <= 0 || H <= 0 || K % 8 || H % 8) throw std::invalid_argument(w + ": D / O and H must be positive multiples of 8");
  if (T < 1) throw std::invalid_argument(w + ": the tile map is empty");
  if (!offsets || !tile_group || !tile_row0 || !n_tiles) throw std::invalid_argument(w + ": missing offsets / tile map");
  uintptr_t bits = 0;
  for (const void* p : ps) {
    if (!p) throw std::invalid_argument(w + ": missing operand");
    bits |= reinterpret_cast<uintptr_t>(p);
  }
  if (bits & 15) throw std::invalid_argument(w + ": operands must be 16-byte aligned");
  const int64_t nwg = static_cast<int64_t>(T) * ((H + QN - 1) / QN);
  if (nwg >= (int64_t(1) << 31)) throw std::invalid_argument(w + ": grid too large");
  return static_cast<unsigned>(nwg);
}

}  // namespace

void grouped_gemm_swiglu(const void* xs, const void* w1, void* gu, void* h, const int* offsets, const int* tile_group,
                         const int* tile_row0, const int* n_tiles, int El, int T, int D, int H, hipStream_t st) {
  const unsigned nwg =
      check_grouped("grouped_gemm_swiglu", {xs, w1, gu, h}, offsets, tile_group, tile_row0, n_tiles, El, T, D, H);
  MoeSwigluArgs g{static_cast<const bf16*>(xs), static_cast<const bf16*>(w1), nullptr, static_cast<bf16*>(gu),
                  static_cast<bf16*>(h), offsets, tile_group, tile_row0, n_tiles, T, D, H};
  hipLaunchKernelGGL(grouped_gemm_swiglu_kernel, dim3(nwg), dim3(QNT), 0, st, g);
  FFK_LAUNCH_CHECK("grouped_gemm_swiglu");
}

void grouped_gemm_swiglu_bwd(const void* dy, const void* w2, const void* gu, void* dgu, const int* offsets,
                             const int* tile_group, const int* tile_row0, const int* n_tiles, int El, int T, int O,
                             int H, hipStream_t st) {
  const unsigned nwg =
      check_grouped("grouped_gemm_swiglu_bwd", {dy, w2, gu, dgu}, offsets, tile_group, tile_row0, n_tiles, El, T, O, H);
  MoeSwigluArgs g{static_cast<const bf16*>(dy), static_cast<const bf16*>(w2), static_cast<const bf16*>(gu),
                  static_cast<bf16*>(dgu), nullptr, offsets, tile_group, tile_row0, n_tiles, T, O, H};
  hipLaunchKernelGGL(grouped_gemm_swiglu_bwd_kernel, dim3(nwg), dim3(QNT), 0, st, g);
  FFK_LAUNCH_CHECK("grouped_gemm_swiglu_bwd");
}

}  // namespace ffk
