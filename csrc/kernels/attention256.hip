// Flash attention for head dimension 256 (forward, dQ, dK/dV) on gfx950, bf16
// in / out, fp32 accumulation and softmax.  Gemma / GPT-J heads, and what
// LlamaConfig(hidden_size=1024, num_heads=4) builds.
//
// The D = 64 / 128 templates of attention.hip keep a wave's accumulators over
// the whole head width; at 256 the dQ and dK/dV forms would need more than
// the 512 registers of a lane.  The kernels here split the work differently.
// Shared with attention.hip (attention_common.h, mfma.h): the strided
// [B, S, H, D] views, the log2-domain LSE [B, H, Sq], delta = rowsum(dO * O)
// taken in the dQ kernel from the dO fragments it already holds,
// v_mfma_f32_32x32x16_bf16 with its fragment layouts, the swizzled LDS images
// and the 16-byte row store.  All three kernels run one workgroup (4 waves)
// per CU, __launch_bounds__(256, 1): 512 registers per lane, the accumulators
// in AGPRs, no scratch (profiles/attn_d256.txt).
//
// LDS images.  A 64-row x 256-column bf16 tile (32 KiB) is kept as two
// 16 KiB sub-images of 256-byte rows, columns 0..127 and 128..255, so the
// 256-byte swizzle of mfma.h (conflict-free for row reads and for
// ds_read_b64_tr_b16) serves it unchanged.  The kernels of the project use
// up to 160 KiB of static LDS per workgroup (gemmpp.hip); the forward takes
// 128 KiB, the dQ kernel 136 KiB, the dK/dV kernel 145 KiB.
//
// Forward (attn256_fwd_kernel).  A workgroup owns 128 queries of one (batch,
// head), a wave 32 whole rows, so the online-softmax state never crosses
// waves: S^T = K Q^T puts one query on a lane, O^T = V^T P^T takes the S^T
// accumulator as its B operand (no LDS round trip for P), the 32 x 256 fp32
// O^T accumulator is 128 registers.  K and V tiles of 64 keys stream through
// a double buffer (4 x 32 KiB), the next tile's loads issued ahead of the
// current tile's MFMAs, one barrier per tile; causal blocks stop at the
// diagonal and run longest first.  Q is held as 64 registers of fragments
// and NOT kept in LDS: next to the 128 KiB of K / V buffers a 128 x 256 Q
// image (64 KiB) does not fit in 160 KiB, and read from LDS it would double
// the LDS bytes per S MFMA (1 KiB of K + 1 KiB of Q per wave and MFMA) on a
// kernel whose LDS reads already match its MFMA time; with one wave per SIMD
// the registers are there (o 128 + q 64 + s 32 + staging 32: one set of
// staging registers carries the next K tile under the S MFMAs and then the
// next V tile under the P V MFMAs; with a set each the kernel spilled).
//
// Backward: the two-phase split, per (64-query tile, 64-key tile).
//  1. The four waves split the 64 x 64 score tile into 32 x 32 quarters.  A
//     wave runs the full 256-deep contractions S = Q K^T and dP = dO V^T of
//     its quarter once (32 MFMAs), forms P = exp2(S c - lse) and dS = P (dP -
//     delta) and writes bf16 images of them to LDS (8 KiB each).
//  2. Each wave owns a 64-column slice of the head dimension and runs the
//     wide products over the whole 64 x 64 tile: two 64 x 64 fp32 accumulators
//     (128 registers) in the dK/dV kernel, one in the dQ kernel.
//  Scores are computed once per kernel and no accumulator is wider than 64
//  columns.  The operands of the resident side sit in registers (dQ: the Q
//  and dO fragments of the wave's 32 queries; dK/dV: the K and V fragments of
//  its 32 keys, 128 registers), the streamed side goes through a double
//  buffer (K / V tiles in the dQ kernel, Q / dO tiles in the dK/dV kernel),
//  staged global -> registers -> LDS around the MFMAs.  Two barriers per tile:
//  after the P / dS images are written, and after phase 2 has read them.
//  * dQ (attn256_bwd_dq_kernel): a workgroup owns 64 queries of one (batch,
//    head).  Phase 1 computes S^T / dP^T (query on the lane, so lse and delta
//    are per-lane scalars) and writes dS as [q][key]; phase 2 is dQ^T[slice]
//    += K^T[slice] dS^T with K^T from transposed reads of the K image.
//  * dK/dV (attn256_bwd_dkdv_kernel): a workgroup owns 64 keys of one
//    (batch, K / V head) and walks the query tiles of every query head of its
//    group as one flat (head, tile) sequence; the accumulators stay in fp32
//    over the group and round once.  Phase 1 computes S / dP with the key on
//    the lane and writes P^T and dS^T as [key][q]; lse and delta of the tile's
//    64 queries travel through LDS with the tile.  Phase 2 is dV^T[slice] +=
//    dO^T[slice] P and dK^T[slice] += Q^T[slice] dS.  Runs after the dQ
//    kernel, which writes delta.
//  No atomics, no workspace: every output element is written by one
//  workgroup, and two calls give equal bits.
//
// Grouped-query K / V: Hkv divides H, query head h reads K / V head h / G,
// G = H / Hkv.  Forward and dQ only index the K / V head; Hkv == H is G = 1.
// Masks: keys >= Sk, queries >= Sq (tail tiles load zeros, are masked, and
// are never stored) and, causal, key > query; causal tiles above the diagonal
// are skipped.  Everything else (dropout, kv_lens / q_lens, seg_lens, bias /
// bias_grad, window, the fused dbias) is refused before any launch.
#include <type_traits>

#include "attention_common.h"
#include "kernels.h"

namespace ffk {

namespace {

struct Attn256Params {
  TensorView q, k, v, o, dout;
  OutView o_out, dq, dk, dv;
  float* lse;    // [B, H, Sq] log2-domain
  float* delta;  // [B, H, Sq]
  int B, H, Hkv, G, Sq, Sk;
  float scale, scale_log2, inv_scale_log2;
};

constexpr int kD = 256;
constexpr int kSub = 64 * 256;   // bytes of a sub-image: 64 rows x 128 columns
constexpr int kTile = 2 * kSub;  // a 64 x 256 tile
constexpr int kPImg = 64 * 128;  // a 64 x 64 bf16 image of P or dS

// Byte offset of 16-byte chunk c (0..31) of row r of a tile.
__device__ __forceinline__ int tile_off(int r, int c) { return (c >> 4) * kSub + img_off<256>(r, c & 15); }

// Global [64][256] tile -> registers -> LDS image: 8 chunks of 16 B per
// thread, a 512-byte row per 32 threads.  Rows >= nrows load zeros.
struct TileStage {
  bf16x8 reg[8];
  __device__ __forceinline__ void load(const TensorView& t, int b, int h, int row0, int nrows) {
    const int ch = threadIdx.x & 31, r0 = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = row0 + r0 + 8 * i;
      reg[i] = r < nrows ? *reinterpret_cast<const bf16x8*>(t.row(b, r, h) + ch * 8) : bf16x8{};
    }
  }
  __device__ __forceinline__ void store(unsigned char* img) const {
    const int ch = threadIdx.x & 31, r0 = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<bf16x8*>(img + tile_off(r0 + 8 * i, ch)) = reg[i];
  }
};

// Row-read fragment of k-step ks (0..15) of a tile: image[row][16 ks + 8 h .. + 8].
__device__ __forceinline__ bf16x8 tile_row_frag(const unsigned char* img, int row, int ks, int h) {
  return lds_read16(img, tile_off(row, 2 * ks + h));
}

// Registers 4g .. 4g+3 of a quarter's accumulator as four bf16, 8 bytes of an
// image row: chunk c of `row`, the lane half's 4 h .. 4 h + 3.
__device__ __forceinline__ void put4(unsigned char* img, int row, int c, int h, float a, float b, float cc, float d) {
  bf16x4 w = {f2bf(a), f2bf(b), f2bf(cc), f2bf(d)};
  *reinterpret_cast<bf16x4*>(img + img_off<128>(row, c) + 8 * h) = w;
}

// ===========================================================================
template <bool CAUSAL>
__global__ __launch_bounds__(256, 1) void attn256_fwd_kernel(Attn256Params P) {
  constexpr int KS = kD / 16, DT = kD / 32, KV = 64;
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * kTile];  // K0 V0 K1 V1

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  // causal: grid (B*H, q blocks), the heaviest query block of a head first
  int bh = blockIdx.x, qb = gridDim.y - 1 - blockIdx.y;
  if (!CAUSAL) attn_head_block(bh, qb);
  const int b = bh / P.H, hh = bh % P.H, hk = hh / P.G;
  const int q_blk = qb * 128;
  const int qw = q_blk + wave * 32;
  const int q = qw + (lane & 31);
  const bool q_ok = q < P.Sq;

  // Q as the B operand of S^T = K Q^T: lane holds Q[q][16 ks + 8 h .. + 8]
  bf16x8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    qf[ks] = q_ok ? *reinterpret_cast<const bf16x8*>(P.q.row(b, q, hh) + ks * 16 + 8 * h) : bf16x8{};

  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x16{};
  float m = -INFINITY, l = 0.f;

  int n_tiles = (P.Sk + KV - 1) / KV;
  if (CAUSAL) n_tiles = min(n_tiles, (q_blk + 128 + KV - 1) / KV);

  // one set of staging registers serves both tiles: the next K tile travels
  // under the S MFMAs, the next V tile under the softmax and the P V MFMAs
  TileStage stg;
  stg.load(P.k, b, hk, 0, P.Sk);
  stg.store(smem);
  stg.load(P.v, b, hk, 0, P.Sk);
  stg.store(smem + kTile);
  __syncthreads();

  for (int t = 0; t < n_tiles; ++t) {
    const int k0 = t * KV;
    const unsigned char* Kt = smem + (t & 1) * 2 * kTile;
    const unsigned char* Vt = Kt + kTile;
    const bool has_next = t + 1 < n_tiles;
    unsigned char* const nxt = smem + ((t + 1) & 1) * 2 * kTile;  // last read in tile t - 1
    if (has_next) stg.load(P.k, b, hk, k0 + KV, P.Sk);  // HBM loads go out ahead of the MFMAs
    const bool active = !CAUSAL || k0 <= qw + 31;  // a wave-uniform skip of the tiles above the wave's diagonal
    f32x16 s[2];
    if (active) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        s[kt] = f32x16{};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s[kt] = mfma32(tile_row_frag(Kt, kt * 32 + (lane & 31), ks, h), qf[ks], s[kt]);
        __builtin_amdgcn_sched_barrier(0);  // the K fragments of one 32-key half at a time (64 registers)
      }
    }
    if (has_next) {
      stg.store(nxt);
      stg.load(P.v, b, hk, k0 + KV, P.Sk);
    }
    if (active) {
      // mask only the tiles that cross the sequence end or the diagonal
      if (k0 + KV > P.Sk || (CAUSAL && k0 + KV - 1 > qw)) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + kt * 32 + acc_row(r) + 4 * h;
            if (key >= P.Sk || (CAUSAL && key > q)) s[kt][r] = -INFINITY;
          }
      }
      float t0 = fmax3(s[0][0], s[0][1], s[0][2]);
      float t1 = fmax3(s[1][0], s[1][1], s[1][2]);
#pragma unroll
      for (int r = 3; r < 15; r += 2) {
        t0 = fmax3(t0, s[0][r], s[0][r + 1]);
        t1 = fmax3(t1, s[1][r], s[1][r + 1]);
      }
      float tmax = fmax3(fmax3(t0, s[0][15], s[1][15]), t1, t1);
      const float tother = __shfl_xor(tmax, 32, 64);
      tmax = fmax3(tmax, tother, tother);
      // lazy rescale (attention.hip): m moves only when a lane's tile max
      // exceeds it by more than 8 in the log2 domain
      if (__any(tmax > m + 8.f * P.inv_scale_log2)) {
        const float m_new = fmaxf(m, tmax);
        const float alpha = (m_new == -INFINITY) ? 1.f : fexp2((m - m_new) * P.scale_log2);
        m = m_new;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] *= alpha;
      }
      const float mc = (m == -INFINITY) ? 0.f : m * P.scale_log2;
      float psum[2] = {0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pv = fexp2(fmaf(s[kt][r], P.scale_log2, -mc));
          s[kt][r] = pv;
          psum[kt] += pv;
        }
      l += psum[0] + psum[1];
      // O^T[d][q] += V^T[d][key] P^T[key][q]
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const bf16x8 pf = acc_to_frag(s[kt], st);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
            o[dt] = mfma32(tr_frag_acc<256>(Vt + (dt >> 2) * kSub, kt * 32 + 16 * st, (dt & 3) * 32, lane), pf, o[dt]);
          // V^T fragments are fetched one k-step ahead at the most: hoisted over
          // all four steps they took 128 registers and the kernel spilled
          __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (has_next) stg.store(nxt + kTile);
    __syncthreads();
  }

  const float lt = l + __shfl_xor(l, 32, 64);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  // the output addresses are formed here from an opaque copy of the row: formed
  // from q and h themselves they were hoisted above the tile loop and spilled across it
  int qe = q, he = h;
  asm volatile("" : "+v"(qe), "+v"(he));
  const bool e_ok = qe < P.Sq;
  store_rows16<DT>(P.o_out.row(b, qe, hh), o, inv, he, e_ok);
  if (e_ok && he == 0)
    P.lse[static_cast<int64_t>(bh) * P.Sq + qe] = (lt > 0.f) ? m * P.scale_log2 + log2f(lt) : -INFINITY;
}

// ===========================================================================
// dQ: 64 queries of one (batch, head) resident, 64-key tiles streamed.
template <bool CAUSAL>
__global__ __launch_bounds__(256, 1) void attn256_bwd_dq_kernel(Attn256Params P) {
  constexpr int KS = kD / 16, KV = 64;
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * kTile + kPImg];  // K0 V0 K1 V1 dS
  unsigned char* const dS = smem + 4 * kTile;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  const int qh = wave & 1, kh = wave >> 1;  // phase 1: the wave's quarter of the score tile
  int bh = blockIdx.x, qb = gridDim.y - 1 - blockIdx.y;
  if (!CAUSAL) attn_head_block(bh, qb);
  const int b = bh / P.H, hh = bh % P.H, hk = hh / P.G;
  const int q_blk = qb * 64;
  const int qw = q_blk + qh * 32;
  const int q = qw + (lane & 31);
  const bool q_ok = q < P.Sq;

  bf16x8 qf[KS], df[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = q_ok ? *reinterpret_cast<const bf16x8*>(P.q.row(b, q, hh) + ks * 16 + 8 * h) : bf16x8{};
    df[ks] = q_ok ? *reinterpret_cast<const bf16x8*>(P.dout.row(b, q, hh) + ks * 16 + 8 * h) : bf16x8{};
  }
  // a dead row takes lse = +inf: P = exp2(-inf) = 0
  const float lse = q_ok ? P.lse[static_cast<int64_t>(bh) * P.Sq + q] : INFINITY;
  // delta = rowsum(dO * O): the lane's d chunks, then the other half's from lane ^ 32
  float part = 0.f;
  if (q_ok) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 of = *reinterpret_cast<const bf16x8*>(P.o.row(b, q, hh) + ks * 16 + 8 * h);
#pragma unroll
      for (int e = 0; e < 8; ++e) part += bf2f(of[e]) * bf2f(df[ks][e]);
    }
  }
  const float dlt = part + __shfl_xor(part, 32, 64);
  if (q_ok && h == 0 && kh == 0) P.delta[static_cast<int64_t>(bh) * P.Sq + q] = dlt;

  // phase 2: dQ^T[d slice of the wave][64 queries], [query tile][d tile]
  f32x16 dq[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) dq[i][j] = f32x16{};
  const int sub = (wave >> 1) * kSub, x0 = (wave & 1) * 64;  // the slice's place in a tile image

  int n_tiles = (P.Sk + KV - 1) / KV;
  if (CAUSAL) n_tiles = min(n_tiles, (q_blk + 64 + KV - 1) / KV);

  TileStage kl, vl;
  kl.load(P.k, b, hk, 0, P.Sk);
  vl.load(P.v, b, hk, 0, P.Sk);
  kl.store(smem);
  vl.store(smem + kTile);
  __syncthreads();

  for (int t = 0; t < n_tiles; ++t) {
    const int k0 = t * KV;
    const unsigned char* Kt = smem + (t & 1) * 2 * kTile;
    const unsigned char* Vt = Kt + kTile;
    const bool has_next = t + 1 < n_tiles;
    if (has_next) {
      kl.load(P.k, b, hk, k0 + KV, P.Sk);
      vl.load(P.v, b, hk, k0 + KV, P.Sk);
    }
    // ---- phase 1: dS of the wave's quarter (keys k0 + 32 kh .., queries qw ..)
    const int kq = k0 + kh * 32;
    f32x16 s = f32x16{}, dp = f32x16{};
    if (!CAUSAL || kq <= qw + 31) {  // a quarter above the diagonal stays zero
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s = mfma32(tile_row_frag(Kt, kh * 32 + (lane & 31), ks, h), qf[ks], s);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) dp = mfma32(tile_row_frag(Vt, kh * 32 + (lane & 31), ks, h), df[ks], dp);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kq + acc_row(r) + 4 * h;
        const float p = fexp2(fmaf(s[r], P.scale_log2, -lse));
        s[r] = (key >= P.Sk || (CAUSAL && key > q)) ? 0.f : p * (dp[r] - dlt);
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
      put4(dS, qh * 32 + (lane & 31), kh * 4 + g, h, s[4 * g], s[4 * g + 1], s[4 * g + 2], s[4 * g + 3]);
    __syncthreads();
    // ---- phase 2: dQ^T[slice][q] += K^T[slice][key] dS^T[key][q]
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 kt[2], ds[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) kt[j] = tr_frag_nat<256>(Kt + sub, 16 * ks, x0 + 32 * j, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i) ds[i] = row_frag<128>(dS, 32 * i, 16 * ks, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) dq[i][j] = mfma32(kt[j], ds[i], dq[i][j]);
    }
    if (has_next) {
      unsigned char* nxt = smem + ((t + 1) & 1) * 2 * kTile;
      kl.store(nxt);
      vl.store(nxt + kTile);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int qr = q_blk + 32 * i + (lane & 31);
    store_rows16<2>(P.dq.row(b, qr, hh) + 64 * wave, dq[i], P.scale, h, qr < P.Sq);
  }
}

// ===========================================================================
// dK/dV: 64 keys of one (batch, K / V head) resident, the 64-query tiles of
// the group's query heads streamed as one flat (head, tile) sequence.
template <bool CAUSAL>
__global__ __launch_bounds__(256, 1) void attn256_bwd_dkdv_kernel(Attn256Params P) {
  constexpr int KS = kD / 16, QT = 64;
  // Q0 dO0 Q1 dO1, P^T, dS^T, then lse / delta of the two staged tiles
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * kTile + 2 * kPImg + 4 * QT * 4];
  unsigned char* const PT = smem + 4 * kTile;
  unsigned char* const dST = PT + kPImg;
  float* const stat = reinterpret_cast<float*>(dST + kPImg);  // [buffer][lse | delta][64]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  const int qh = wave & 1, kh = wave >> 1;  // phase 1: the wave's quarter of the score tile
  // causal: grid (B*Hkv, key blocks); key block 0 sees every query tile and goes first
  int bh = blockIdx.x, kb = blockIdx.y;
  if (!CAUSAL) attn_head_block(bh, kb);
  const int b = bh / P.Hkv, hk = bh % P.Hkv;
  const int k_blk = kb * 64;
  const int key = k_blk + kh * 32 + (lane & 31);
  const bool key_ok = key < P.Sk;

  // K and V of the lane's key as the B operands of S = Q K^T and dP = dO V^T
  bf16x8 kf[KS], vf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = key_ok ? *reinterpret_cast<const bf16x8*>(P.k.row(b, key, hk) + ks * 16 + 8 * h) : bf16x8{};
    vf[ks] = key_ok ? *reinterpret_cast<const bf16x8*>(P.v.row(b, key, hk) + ks * 16 + 8 * h) : bf16x8{};
  }
  // phase 2: dV^T / dK^T[d slice of the wave][64 keys], [key tile][d tile]
  f32x16 dv[2][2], dk[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) dv[i][j] = dk[i][j] = f32x16{};
  const int sub = (wave >> 1) * kSub, x0 = (wave & 1) * 64;

  // query tiles t_lo .. t_hi of every head of the group; causal starts at the diagonal
  const int t_hi = (P.Sq + QT - 1) / QT;
  const int t_lo = CAUSAL ? min(k_blk / QT, t_hi) : 0;
  const int per_head = t_hi - t_lo, steps = per_head * P.G;

  TileStage ql, dl;
  float st_lse = 0.f, st_dlt = 0.f;  // threads 0..63: lse / delta of the staged tile's row
  auto load = [&](int g, int t) {
    const int hq = hk * P.G + g, q0 = t * QT;
    ql.load(P.q, b, hq, q0, P.Sq);
    dl.load(P.dout, b, hq, q0, P.Sq);
    if (threadIdx.x < QT) {
      const bool ok = q0 + static_cast<int>(threadIdx.x) < P.Sq;
      const int64_t i = (static_cast<int64_t>(b) * P.H + hq) * P.Sq + q0 + threadIdx.x;
      st_lse = ok ? P.lse[i] : INFINITY;  // a dead row: P = exp2(-inf) = 0
      st_dlt = ok ? P.delta[i] : 0.f;
    }
  };
  auto store = [&](int buf) {
    ql.store(smem + buf * 2 * kTile);
    dl.store(smem + buf * 2 * kTile + kTile);
    if (threadIdx.x < QT) {
      stat[buf * 2 * QT + threadIdx.x] = st_lse;
      stat[buf * 2 * QT + QT + threadIdx.x] = st_dlt;
    }
  };
  if (steps > 0) {
    load(0, t_lo);
    store(0);
  }
  __syncthreads();

  int g = 0, t = t_lo;
  for (int i = 0; i < steps; ++i) {
    const int buf = i & 1;
    const unsigned char* Qt = smem + buf * 2 * kTile;
    const unsigned char* Dt = Qt + kTile;
    int gn = g, tn = t + 1;
    if (tn == t_hi) tn = t_lo, ++gn;
    const bool has_next = i + 1 < steps;
    if (has_next) load(gn, tn);
    // ---- phase 1: P and dS of the wave's quarter (queries q0 + 32 qh .., keys of the lanes)
    const int qq = t * QT + qh * 32;
    f32x16 s = f32x16{}, dp = f32x16{};
    const bool live = !CAUSAL || k_blk + kh * 32 <= qq + 31;  // a quarter above the diagonal stays zero
    if (live) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s = mfma32(tile_row_frag(Qt, qh * 32 + (lane & 31), ks, h), kf[ks], s);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) dp = mfma32(tile_row_frag(Dt, qh * 32 + (lane & 31), ks, h), vf[ks], dp);
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const f32x4 ls = *reinterpret_cast<const f32x4*>(stat + buf * 2 * QT + qh * 32 + 8 * gq + 4 * h);
        const f32x4 dt = *reinterpret_cast<const f32x4*>(stat + buf * 2 * QT + QT + qh * 32 + 8 * gq + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * gq + e, qr = qq + 8 * gq + 4 * h + e;
          const bool dead = !key_ok || (CAUSAL && key > qr);
          const float p = dead ? 0.f : fexp2(fmaf(s[r], P.scale_log2, -ls[e]));
          s[r] = p;
          dp[r] = p * (dp[r] - dt[e]);
        }
      }
    }
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      put4(PT, kh * 32 + (lane & 31), qh * 4 + gq, h, s[4 * gq], s[4 * gq + 1], s[4 * gq + 2], s[4 * gq + 3]);
      put4(dST, kh * 32 + (lane & 31), qh * 4 + gq, h, dp[4 * gq], dp[4 * gq + 1], dp[4 * gq + 2], dp[4 * gq + 3]);
    }
    __syncthreads();
    // ---- phase 2: dV^T[slice][key] += dO^T[slice][q] P[q][key], dK^T[slice][key] += Q^T[slice][q] dS[q][key]
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 a[2], bb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) a[j] = tr_frag_nat<256>(Dt + sub, 16 * ks, x0 + 32 * j, lane);
#pragma unroll
      for (int k = 0; k < 2; ++k) bb[k] = row_frag<128>(PT, 32 * k, 16 * ks, lane);
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 2; ++j) dv[k][j] = mfma32(a[j], bb[k], dv[k][j]);
#pragma unroll
      for (int j = 0; j < 2; ++j) a[j] = tr_frag_nat<256>(Qt + sub, 16 * ks, x0 + 32 * j, lane);
#pragma unroll
      for (int k = 0; k < 2; ++k) bb[k] = row_frag<128>(dST, 32 * k, 16 * ks, lane);
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 2; ++j) dk[k][j] = mfma32(a[j], bb[k], dk[k][j]);
    }
    if (has_next) store(buf ^ 1);
    __syncthreads();
    g = gn, t = tn;
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int kr = k_blk + 32 * k + (lane & 31);
    store_rows16<2>(P.dv.row(b, kr, hk) + 64 * wave, dv[k], 1.f, h, kr < P.Sk);
    store_rows16<2>(P.dk.row(b, kr, hk) + 64 * wave, dk[k], P.scale, h, kr < P.Sk);
  }
}

// What the D = 256 kernels do not serve, refused by name before any launch.
Attn256Params make_params256(const AttnTensors& t, int B, int H, int Sq, int Sk, float scale, bool causal, bool bwd) {
  auto refuse = [](const char* what) {
    throw std::invalid_argument(std::string("attention: head dim 256 excludes ") + what);
  };
  if (t.drop_threshold) refuse("dropout");
  if (t.kv_lens) refuse("kv_lens");
  if (t.q_lens) refuse("q_lens");
  if (t.seg_offsets) refuse("packed sequences (seg_lens)");
  if (t.bias.p) refuse("bias");
  if (t.bias_grad.p) refuse("bias_grad");
  if (t.window) refuse("window");
  if (t.dbq || t.dbk || t.dbv) refuse("the fused dbias");
  Attn256Params P{};
  P.Hkv = t.kv_heads > 0 ? t.kv_heads : H;
  if (t.kv_heads < 0 || H % P.Hkv)
    throw std::invalid_argument("attention: grouped-query K / V heads (kv_heads) must divide the query heads H");
  P.G = H / P.Hkv;
  if (B < 1 || H < 1 || Sq < 1 || Sk < 1) throw std::invalid_argument("attention: head dim 256 needs B, H, Sq, Sk >= 1");
  const int64_t cols = static_cast<int64_t>(B) * H, rows = (Sq + 63) / 64 > (Sk + 63) / 64 ? (Sq + 63) / 64 : (Sk + 63) / 64;
  if (causal ? rows > 65535 : cols > 65535) throw std::invalid_argument("attention: head dim 256: the call exceeds the grid");
  // 16-byte vector accesses: aligned bases, strides that are multiples of 8 elements
  auto aligned = [](const AttnTensors::T& x) {
    return !x.p || (reinterpret_cast<uintptr_t>(x.p) % 16 == 0 && x.sb % 8 == 0 && x.ss % 8 == 0 && x.sh % 8 == 0);
  };
  if (!aligned(t.q) || !aligned(t.k) || !aligned(t.v) || !aligned(t.o) || !aligned(t.dout) || !aligned(t.dq) ||
      !aligned(t.dk) || !aligned(t.dv))
    throw std::invalid_argument("attention: head dim 256 needs 16-byte aligned views (strides that are multiples of 8)");
  if (!t.q.p || !t.k.p || !t.v.p || !t.o.p || !t.lse || (bwd && (!t.dout.p || !t.dq.p || !t.dk.p || !t.dv.p || !t.delta)))
    throw std::invalid_argument("attention: head dim 256: a tensor of the call is missing");
  auto tv = [](const AttnTensors::T& x) { return TensorView{static_cast<const bf16*>(x.p), x.sb, x.ss, x.sh}; };
  auto ov = [](const AttnTensors::T& x) {
    return OutView{static_cast<bf16*>(const_cast<void*>(x.p)), x.sb, x.ss, x.sh};
  };
  P.q = tv(t.q); P.k = tv(t.k); P.v = tv(t.v); P.o = tv(t.o); P.dout = tv(t.dout);
  P.o_out = ov(t.o); P.dq = ov(t.dq); P.dk = ov(t.dk); P.dv = ov(t.dv);
  P.lse = t.lse;
  P.delta = t.delta;
  P.B = B; P.H = H; P.Sq = Sq; P.Sk = Sk;
  P.scale = scale;
  P.scale_log2 = scale * kLog2e;
  P.inv_scale_log2 = 1.f / P.scale_log2;
  return P;
}

}  // namespace

void attention256_fwd(const AttnTensors& t, int B, int H, int Sq, int Sk, float scale, bool causal, hipStream_t st) {
  const Attn256Params P = make_params256(t, B, H, Sq, Sk, scale, causal, false);
  const unsigned nq = static_cast<unsigned>((Sq + 127) / 128), nbh = static_cast<unsigned>(B * H);
  if (causal) hipLaunchKernelGGL(attn256_fwd_kernel<true>, dim3(nbh, nq), dim3(256), 0, st, P);
  else hipLaunchKernelGGL(attn256_fwd_kernel<false>, dim3(nq, nbh), dim3(256), 0, st, P);
  FFK_LAUNCH_CHECK("attention_fwd (head dim 256)");
}

void attention256_bwd(const AttnTensors& t, int B, int H, int Sq, int Sk, float scale, bool causal, hipStream_t st) {
  const Attn256Params P = make_params256(t, B, H, Sq, Sk, scale, causal, true);
  const unsigned nq = static_cast<unsigned>((Sq + 63) / 64), nk = static_cast<unsigned>((Sk + 63) / 64);
  const unsigned nbh = static_cast<unsigned>(B * H), nkh = static_cast<unsigned>(B * P.Hkv);
  // dQ first: it writes the delta that the dK / dV kernel reads
  if (causal) {
    hipLaunchKernelGGL(attn256_bwd_dq_kernel<true>, dim3(nbh, nq), dim3(256), 0, st, P);
    hipLaunchKernelGGL(attn256_bwd_dkdv_kernel<true>, dim3(nkh, nk), dim3(256), 0, st, P);
  } else {
    hipLaunchKernelGGL(attn256_bwd_dq_kernel<false>, dim3(nq, nbh), dim3(256), 0, st, P);
    hipLaunchKernelGGL(attn256_bwd_dkdv_kernel<false>, dim3(nk, nkh), dim3(256), 0, st, P);
  }
  FFK_LAUNCH_CHECK("attention_bwd (head dim 256)");
}

}  // namespace ffk
