// Flash attention (forward + backward) for gfx950, bf16 in / fp32 accumulate.
//
// Parity: lib/kernels/src/cuda/ops/attention_kernels.cu, which calls cuDNN's
// monolithic cudnnMultiHeadAttnForward/BackwardData/BackwardWeights (:255,
// :292, :316) and materialises the whole attention matrix.  Here the score
// matrix never leaves the CU (blockwise online softmax), which is what makes
// the long-sequence configs of SURVEY.md §5.7 possible.
//
// CDNA4 design:
//  * MFMA v_mfma_f32_32x32x16_bf16; a workgroup = 4 waves, each wave owns 32
//    query rows (forward, dQ) or 32 key rows (dK/dV).
//  * "swapped" products: the forward computes S^T = K Q^T so every lane holds
//    scores of ONE query -> the row max / row sum are lane-local plus a single
//    exchange with lane^32; O^T = V^T P^T consumes the S^T accumulator
//    directly as the MFMA B operand (accumulator-as-operand, no LDS round
//    trip for P) and keeps the query on the lane, so the online-softmax
//    rescale is a per-lane scalar multiply.
//  * K/V tiles are staged global->registers->LDS with the next tile's loads
//    issued before the current tile's MFMAs (async-STAGE split, T14), double
//    buffered, one barrier per tile.
//  * LDS images are XOR-swizzled per row so ds_read_b128 row reads are
//    conflict-free; V^T (and K^T / Q^T / dO^T in the backward) operands come
//    from ds_read_b64_tr_b16 hardware-transposed reads of the same images.
//  * output rows leave as 16-byte stores (store_rows16), and non-causal grids
//    visit the heads in XCD-local order (attn_head_block).
//  * backward = dQ kernel (query block resident; also computes delta =
//    rowsum(dO*O) for its queries) then dK/dV kernel (key block resident,
//    loops over query tiles, key on the lane) -> no float atomics,
//    deterministic, no [N, N] buffers.  Non-causal D = 64 calls with at most
//    512 keys take the one-pass kernel instead (attn_bwd_onepass_kernel): one
//    workgroup per (batch, head), all three gradients from one S / dS.
//
// Kernels: attn_fwd_kernel, attn_bwd_dq_kernel and attn_bwd_dkdv_kernel, each
// for D in {64, 128} x CAUSAL x DROP x VARLEN (and, with VARLEN, PACKED) plus
// D x DROP with BIAS and D x CAUSAL with GQA, and attn_bwd_onepass_kernel;
// attention_fwd / attention_bwd pick one through with_head and
// with_features.  Packed calls also launch
// attn_segment_offsets_kernel (before) and attn_pack_tail_kernel (after).
// Two environment switches: FFK_ATTN_PRIO (wave priority around the MFMA
// clusters; default on at D = 128) and FFK_ATTN_BWD_ONEPASS (0: the kernel
// pair where the one-pass kernel would run; read per call).
//
// Tensor addressing: every tensor is [B, S, H, D] with arbitrary strides for
// b / s / h and contiguous d (TensorViewT::row), so the fused QKV projection
// output [B, S, 3, H, D] is consumed in place.  LSE is [B, H, S] fp32, log2
// domain.
//
// Attention dropout (DROP instantiations of the forward, dQ and dK/dV
// kernels).  The keep / drop decision of probability (b, h, q, k) is a pure
// function of (seed, b, h, q, k, T), independent of tiling, kernel, wave
// layout and strides; every kernel regenerates it and nothing of size
// Sq x Sk is stored.  The definition (ops/attention.py attention_dropout_mask
// is its second implementation):
//   seed_eff = seed + *seed_dev (mod 2^64; seed alone without a device word)
//   key      = hash_u32(seed_eff, b * H + h)      splitmix64 finaliser, low 32
//                                                 bits; once per workgroup
//   x        = mix32((q * Sk + k) ^ key)          needs Sq * Sk < 2^32
//   mix32:     x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
//              x ^= x >> 16
//   keep iff (x >> 8) >= T,  T = round(p * 2^24) from the host
// Kept probabilities are scaled by rs = 2^24 / (2^24 - T), exactly unbiased
// for the realised rate.  m, l and the LSE come from the undropped
// probabilities (the LSE is that of a p = 0 call); O = rs (keep . P) V, so
// delta = rowsum(dO * O) is unchanged and dS = P (keep rs dP - delta),
// dV = rs (keep . P)^T dO.
//
// Per-sample key lengths (VARLEN instantiations of the forward, dQ and dK/dV
// kernels; AttnTensors::kv_lens, int32 [B] on the device).  Keys >=
// kv_lens[b] do not exist for sample b: every bound on the key axis (tile
// count, tile loads, masks, the dK/dV wave's key test) takes the sample's
// length, read once per workgroup as a scalar and clamped to [0, Sk], in the
// place of Sk.  Rows past the length are never read (the loaders return
// zeros, as they do past Sk), the forward and dQ kernels stop at the last
// live key tile, a dK/dV workgroup whose key block is wholly dead skips its
// query loop, and dK = dV = 0 is stored for every dead key below the physical
// Sk (the gradient buffers are uninitialised).  A row without a live key gets
// o = 0, lse = -inf and dQ = 0.  The dropout hash index and the dbias slab
// rows keep the physical Sk.  The backward with lengths is the dQ + dK/dV
// pair; a call without lengths runs the VARLEN = false kernels, in which the
// bound is P.Sk as before.
//
// Per-sample query lengths (the same VARLEN instantiations;
// AttnTensors::q_lens, int32 [B] on the device, clamped to [0, Sq]).  Queries
// >= q_lens[b] do not exist for sample b, with the definitions of the key
// axis mirrored: o = 0, lse = -inf and dQ = 0 are stored for every dead row
// below the physical Sq, a dead row adds nothing to dK, dV or the dbias
// partials, and Q, O, dO, lse and delta of a dead row are never read.  A
// forward / dQ workgroup whose 128-query block is wholly dead stores its
// zeros and returns before the tile loop (a workgroup-uniform exit ahead of
// the first barrier); a wholly dead wave of a live block stages tiles and
// meets the barriers without MFMAs, like an inactive causal wave; dead rows
// of a live wave load zeros and are masked.  The dK/dV kernel's query-tile
// loop ends at the last live tile.  Either pointer may be null in a VARLEN
// kernel: null means the physical extent.  The dropout hash index and the
// dbias slab rows keep their physical positions.
//
// Packed sequences (PACKED instantiations, an axis of their own so that the
// kernels of a call with lengths stay the code they were;
// AttnTensors::seg_offsets, int32 [N, M, 2] on the device).  Row n of the
// [N, T, H, D] tensors (a pack) holds up to M sequences (segments) end to end
// from token 0; segment (n, m) is tokens start .. start + len of pack n, with
// (start, len) written by attn_segment_offsets_kernel from seg_lens [N, M]
// (start = sum of the pack's earlier clamped lengths, len clamped to
// [0, min(max_seqlen, T - start)]) once per forward and kept for the backward.
// A workgroup serves one segment: the grid's b is n * M + m over N * M * H
// columns and ceil(max_seqlen / 128) blocks, Sq = Sk = max_seqlen, and the
// segment's len takes the place of both lengths, so every rule above holds in
// segment-local coordinates (causal and the dropout mask included: the hash
// key is that of sample n * M + m, the row stride max_seqlen).  What differs:
//  * every row address is pack base + (start + local row) * stride, and the
//    LSE / delta words are [N, H, T] by physical token;
//  * a dead row of one segment may be a live row of the next, so nothing is
//    stored outside the segment: the dead-block exits store nothing (the
//    dK/dV kernel has one too, ahead of its first barrier), the epilogues
//    store live rows only, and the dK/dV zero stores for dead keys are off.
//    Loaders bound rows by len, so a tile that straddles a segment end reads
//    zeros for the neighbour's rows and leaves them untouched;
//  * the tokens past a pack's last segment (the tail) are written by
//    attn_pack_tail_kernel after the attention kernels: zeros in o / dQ / dK /
//    dV and lse = -inf (the GEMMs around attention reduce over all T rows).
// kv_lens / q_lens, dbias in either form, Sq != Sk and the one-pass backward
// are not part of the packed mode (std::invalid_argument; always the pair).
//
// Additive score bias (BIAS instantiations of the forward, dQ and dK/dV
// kernels, D in {64, 128} with and without DROP, and only with CAUSAL =
// VARLEN = PACKED = false; AttnTensors::bias).  fp32, element strides sb / sh
// / sq for batch / head / query (0 = broadcast over that axis), the key axis
// contiguous.  The score of (b, h, q, k) is scale * q.k + bias[b * sb + h * sh
// + q * sq + k] before the softmax, i.e. in the log2 domain t = s * scale_log2
// + bias * log2(e); -inf masks the pair.
//  * forward: the bias enters as the initial value of the S^T accumulator
//    (S' = K Q^T + bias / scale), so the running max, the lazy-rescale test
//    and exp2 see t = S' * scale_log2 through the code of the unbiased kernel
//    (the max of the raw q.k alone would be wrong).  A row with every key at
//    -inf keeps m = -inf, l = 0: o = 0 and lse = -inf (torch gives NaN); the
//    m == -inf guards keep NaN out on the way.
//  * backward: P = exp2(t - lse).  A row whose lse is -inf has t = -inf
//    everywhere; the dQ kernel takes its lse as +inf and the dK/dV kernel
//    parks S' = -inf for it, so P = 0 (never exp2(-inf + inf)): dQ = 0, and
//    the row adds nothing to dK / dV.  dS = P (keep rs dP - delta) and dQ =
//    scale * dS K are unchanged.  No gradient is produced for the bias.
//  * loads: in the forward and dQ kernels a lane owns one query and its
//    registers hold four consecutive keys per group: one 16-byte load per
//    group (bias_group).  In the dK/dV kernel a lane owns a key and its
//    registers run over queries: 32 lanes read 128 consecutive bytes of a
//    bias row.  The host requires a 16-byte aligned base, Sk % 4 == 0 and
//    sb / sh / sq that are 0 or multiples of 4 (std::invalid_argument), so a
//    group never straddles Sk; keys >= Sk and queries >= Sq are never read.
//  * a tile's bias loads are issued ahead of its MFMAs and on the far side of
//    the K / V (Q / dO) prefetch in issue order: vmcnt retires in order, so
//    the wait for the bias leaves the prefetch in flight.
//  * occupancy: the forward at D = 128 and the dK/dV kernel at D = 64 run one
//    wave per SIMD with a bias (the unbiased forms run two): at two, the
//    tile's 32 bias registers spilled into the tile loop.  No BIAS kernel has
//    scratch (profiles/r7/attn_bias_isa.txt).
//  * masked keys are still READ, unlike keys past kv_lens: K / V content
//    under a mask must be finite (0 * NaN).  The dropout hash index is
//    unchanged, (b * H + h, q * Sk + k).
// Bias excludes causal, kv_lens, q_lens, seg_offsets and the fused dbias
// (std::invalid_argument), and its backward is always the dQ + dK/dV pair.
// A call without a bias runs the BIAS = false kernels, the code they were.
//
// Grouped-query attention (GQA instantiations of the forward, dQ and dK/dV
// kernels, D in {64, 128} x CAUSAL, and only with DROP = VARLEN = PACKED =
// BIAS = false; AttnTensors::kv_heads).  K, V, dK and dV have Hkv heads, Hkv
// dividing H, G = H / Hkv; query head h attends over K / V head h / G (torch's
// enable_gqa, repeat_interleave(G) over the heads), and dK[hk] / dV[hk] are
// the sums of the per-query-head gradients over h in [hk * G, (hk + 1) * G).
//  * forward and dQ: the grid stays over the B * H query heads.  The head of
//    every K / V row address and tile load is hh / G (kv_head), uniform over
//    the workgroup and so a scalar; Q, O, dO, dQ, LSE and delta stay on the
//    query head.  A query head does the arithmetic of the H-head call on the
//    same bits: o, lse and dq equal those of a call on K / V expanded to H
//    heads bit for bit.
//  * dK/dV: the grid is over the B * Hkv K / V heads.  A workgroup loads its
//    K / V fragments once and runs the query-tile loop for each of the G
//    query heads of its group as one flat sequence of (head, tile) steps, so
//    the LDS double buffer and the prefetch run across head boundaries and
//    every barrier stays workgroup-uniform; Q / dO tiles, LSE and delta are
//    those of query head hk * G + g (rows (b * H + hk * G + g) * Sq + q);
//    with CAUSAL each head starts again at the key block's first tile.  dK
//    and dV accumulate in the fp32 registers over the whole group and are
//    stored once, with one bf16 rounding (summing per-head bf16 gradients of
//    an expanded call rounds G + 1 times).
//  * occupancy: __launch_bounds__ are those of the forms without GQA; no GQA
//    kernel has scratch (profiles/r7/attn_gqa_isa.txt).
//  * the dK/dV grid has G times fewer workgroups than an H-head call's, B *
//    Hkv * ceil(Sk / 128); splitting a group over workgroups is not done.
// GQA excludes dropout, kv_lens, q_lens, seg_offsets, bias and the fused dbias
// (std::invalid_argument), and its backward is always the dQ + dK/dV pair.  A
// call with Hkv == H runs the GQA = false kernels, the code they were.
#include <cstdlib>
#include <type_traits>

#include "kernels.h"
#include "mfma.h"

namespace ffk {

// A [B, S, H, D] tensor: element strides for b / s / h, d contiguous.
template <class T>
struct TensorViewT {
  T* p;
  int64_t sb, ss, sh;
  __device__ __forceinline__ T* row(int b, int s, int h) const { return p + b * sb + static_cast<int64_t>(s) * ss + h * sh; }
};
using TensorView = TensorViewT<const bf16>;
using OutView = TensorViewT<bf16>;

struct AttnParams {
  TensorView q, k, v, o, dout;
  OutView o_out, dq, dk, dv;
  float* lse;    // [B, H, Sq] log2-domain
  float* delta;  // [B, H, Sq]
  float *dbq, *dbk, *dbv;  // optional [H*D] projection-bias gradients (column sums of dq / dk / dv)
  int64_t db_ld;           // > 0: dbq / dbk / dbv are per-32-row partial slabs with this row stride
  int B, H, Sq, Sk;
  float scale;       // softmax scale (1/sqrt(D) by default)
  float scale_log2;  // scale * log2(e)
  float inv_scale_log2;  // 1 / scale_log2 (no IEEE divide in the loops)
  int prio;          // raise wave priority around MFMA clusters (FFK_ATTN_PRIO; guide T5)
  // attention dropout (DROP kernels only)
  unsigned drop_thr;        // T << 8: a probability is dropped iff its hash word is below this
  float drop_rs;            // keep scale 2^24 / (2^24 - T)
  uint64_t seed;
  const int64_t* seed_dev;  // optional device-resident addend of the seed
  // per-sample lengths (VARLEN kernels only)
  const int32_t* kv_lens;   // [B]; keys >= kv_lens[b] of sample b do not exist
  const int32_t* q_lens;    // [B]; queries >= q_lens[b] of sample b do not exist
  // packed sequences (PACKED kernels only; B = packs, Sq = Sk = max_seqlen)
  const int32_t* seg_off;   // [B, M, 2]: clamped (start, len) of segment (n, m), from attn_segment_offsets_kernel
  int M, T;                 // segment slots per pack; physical tokens per pack
  // additive score bias (BIAS kernels only): fp32, the key axis contiguous
  const float* bias;
  int64_t bias_sb, bias_sh, bias_sq;  // element strides of batch / head / query, 0 = broadcast
  // grouped-query attention (GQA kernels only): K / V have Hkv heads, G = H / Hkv
  int Hkv, G;
};

constexpr float kLog2e = 1.4426950408889634f;

// Score bias (BIAS kernels): the four consecutive keys kg .. kg + 3 of one
// query's bias row as one 16-byte load.  The host guarantees Sk % 4 == 0 and
// 16-byte aligned rows, so a group lies wholly below Sk or wholly past it;
// groups past Sk and rows past Sq (`ok` false) are never read.
__device__ __forceinline__ f32x4 bias_group(const float* row, int kg, int Sk, bool ok) {
  return (ok && kg < Sk) ? *reinterpret_cast<const f32x4*>(row + kg) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// Row of register r of a 32 x 32 MFMA accumulator, before the lane half's
// + 4 h: registers 4g .. 4g+3 hold rows 8g .. 8g+3.
__device__ constexpr int acc_row(int r) { return (r & 3) + 8 * (r >> 2); }

// Key-axis bound of sample b.  VARLEN: the sample's own length, read from the
// device (so a captured launch follows the tensor) and clamped to [0, Sk] so
// that a bad value cannot read out of bounds; b is uniform over the
// workgroup, which makes this one scalar load.  Otherwise the physical Sk.
// The dropout hash index keeps the physical Sk as its row stride either way.
template <bool VARLEN>
__device__ __forceinline__ int key_len(const AttnParams& P, int b) {
  if constexpr (VARLEN) return P.kv_lens ? __builtin_amdgcn_readfirstlane(min(max(P.kv_lens[b], 0), P.Sk)) : P.Sk;
  else return P.Sk;
}
// Query-axis bound of sample b, the same way: q_lens[b] clamped to [0, Sq] in
// a VARLEN kernel that was given query lengths, otherwise the physical Sq.
template <bool VARLEN>
__device__ __forceinline__ int query_len(const AttnParams& P, int b) {
  if constexpr (VARLEN) return P.q_lens ? __builtin_amdgcn_readfirstlane(min(max(P.q_lens[b], 0), P.Sq)) : P.Sq;
  else return P.Sq;
}

// K / V head of query head hh.  GQA: hh / G, uniform over the workgroup (hh
// derives from the block id), so a scalar.  Otherwise the query head itself.
template <bool GQA>
__device__ __forceinline__ int kv_head(const AttnParams& P, int hh) {
  if constexpr (GQA) return hh / P.G;
  else return hh;
}

// Packed sequences: the segment a workgroup serves.  `b` of the grid is the
// segment n * M + m; its rows are tokens start .. start + len of pack n, and
// the LSE / delta rows are [pack, head, physical token].  Both words are read
// once per workgroup as scalars and clamped again, so that no content of the
// offsets tensor can address outside the pack.
struct Segment {
  int n, start, len;
};
__device__ __forceinline__ Segment segment_of(const AttnParams& P, int b) {
  const int st = min(max(__builtin_amdgcn_readfirstlane(P.seg_off[2 * b]), 0), P.T);
  const int ln = min(max(__builtin_amdgcn_readfirstlane(P.seg_off[2 * b + 1]), 0), min(P.Sq, P.T - st));
  return {b / P.M, st, ln};
}
// Index of a row's LSE / delta word.  `row` is the sample's row, or with
// PACKED the physical token start + local row of pack pn.
template <bool PACKED>
__device__ __forceinline__ int64_t stat_index(const AttnParams& P, int bh, int pn, int hh, int row) {
  if constexpr (PACKED) return (static_cast<int64_t>(pn) * P.H + hh) * P.T + row;
  else return static_cast<int64_t>(bh) * P.Sq + row;
}

// A wave's 32 dead query rows (lane & 31 -> row, lane half h -> the row's odd
// or even 16-byte chunks) stored as zeros: the output of a workgroup that
// leaves before its tile loop.
template <int D>
__device__ __forceinline__ void store_zero_rows(bf16* row, int h) {
#pragma unroll
  for (int c = 0; c < D / 16; ++c) *reinterpret_cast<u32x4t*>(row + (2 * c + h) * 8) = u32x4t{0u, 0u, 0u, 0u};
}

// Dropout hash (definition in the header comment).  drop_key is uniform over
// the workgroup: made a scalar so the per-element xor takes it from an SGPR.
__device__ __forceinline__ unsigned drop_key(const AttnParams& P, int bh) {
  uint64_t seed = P.seed;
  if (P.seed_dev) seed += static_cast<uint64_t>(*P.seed_dev);
  return __builtin_amdgcn_readfirstlane(hash_u32(seed, static_cast<uint64_t>(bh)));
}
__device__ __forceinline__ bool dropped(unsigned idx, unsigned key, unsigned thr) {
  unsigned x = idx ^ key;
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x < thr;  // (x >> 8) < T
}

// Store a wave's 32-row C^T tile (lane & 31 -> row, registers -> d) as rows
// of bf16, 16 bytes per store.  A lane holds 4 consecutive d of each 8-group
// (lane half h: d = 8 g + 4 h + e); v_permlane32_swap trades group 2p+1 of
// the lower half for group 2p of the upper half, so after the swap every
// lane holds 8 consecutive d (lower half: d 16p..16p+7 = its own group 2p
// and its partner's; upper half: 16p+8..16p+15) -- half the store
// instructions of the 8-byte form (the epilogue tail is store-issue bound,
// guide T21).  Every lane runs the swaps; `ok` guards only the stores.
template <int DT>
__device__ __forceinline__ void store_rows16(bf16* row, const f32x16 (&acc)[DT], float mul, int h, bool ok) {
  auto pk = [](float a, float b) -> unsigned {
    return static_cast<unsigned>(f2u(a)) | (static_cast<unsigned>(f2u(b)) << 16);
  };
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      const int ga = 2 * gp, gb = 2 * gp + 1;
      const unsigned xa0 = pk(acc[dt][4 * ga + 0] * mul, acc[dt][4 * ga + 1] * mul);
      const unsigned xa1 = pk(acc[dt][4 * ga + 2] * mul, acc[dt][4 * ga + 3] * mul);
      const unsigned yb0 = pk(acc[dt][4 * gb + 0] * mul, acc[dt][4 * gb + 1] * mul);
      const unsigned yb1 = pk(acc[dt][4 * gb + 2] * mul, acc[dt][4 * gb + 3] * mul);
      const auto s0 = __builtin_amdgcn_permlane32_swap(xa0, yb0, false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(xa1, yb1, false, false);
      if (ok) {
        u32x4t v = {static_cast<unsigned>(s0[0]), static_cast<unsigned>(s1[0]), static_cast<unsigned>(s0[1]),
                    static_cast<unsigned>(s1[1])};
        *reinterpret_cast<u32x4t*>(row + dt * 32 + 16 * gp + 8 * h) = v;
      }
    }
}

// (head, block) of a non-causal workgroup, grid (blocks, B*H).  Dispatch puts
// linear id L = x + y * gridDim.x on XCD L % 8, so without a remap the
// blocks of one head (4 query blocks at S = 512) run on four XCDs and every
// XCD's L2 fetches that head's K / V.  The bijective remap (mfma.h) gives
// each XCD a contiguous range of linear ids, i.e. whole heads: a head's K / V
// come from HBM once and its other blocks hit in the XCD's L2.
__device__ __forceinline__ void attn_head_block(int& bh, int& blk) {
  const int W = gridDim.x * gridDim.y;
  const int r = xcd_remap(blockIdx.x + blockIdx.y * gridDim.x, W);
  bh = r / gridDim.x;
  blk = r % gridDim.x;
}

__device__ __forceinline__ void prio_hi(const AttnParams& P) {
  if (P.prio) __builtin_amdgcn_s_setprio(1);
}
__device__ __forceinline__ void prio_lo(const AttnParams& P) {
  if (P.prio) __builtin_amdgcn_s_setprio(0);
}

template <int D>
__device__ __forceinline__ int lds_off(int r, int c) {  // byte offset of chunk c of row r
  return img_off<D * 2>(r, c);
}
template <int D>
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* img, int row0, int dt, int lane) {
  return tr_frag_acc<D * 2>(img, row0, dt * 32, lane);
}

// Bias gradient of a projection: add the column sums of a wave's 32-row
// output tile (C^T accumulator: lane&31 -> row, registers -> d) times `mul`
// into db[d] — shuffles over the 32 rows of each lane half, then one fp32
// atomic per column (32 per lane half).  Rows outside the sequence must hold
// zeros (they do: masked rows contribute nothing to the accumulators).
template <int DT>
__device__ __forceinline__ void bias_colsum(const f32x16 (&acc)[DT], float mul, float* db, int lane) {
  const int h = lane >> 5;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = acc[dt][r];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if ((lane & 31) == 0) atomicAdd(db + dt * 32 + acc_row(r) + 4 * h, v * mul);
    }
}

// Global [rows][D] tile -> registers (each of NT threads `per` chunks of 16 B).
template <int D, int ROWS, int NT = 256>
struct TileLoader {
  static constexpr int CHUNKS = ROWS * D / 8;
  static constexpr int PER = CHUNKS / NT;
  bf16x8 reg[PER];
  // rows row0 .. of a sample that has nrows; `base` is the sample's first
  // physical row (a packed segment's start)
  __device__ __forceinline__ void load(const TensorView& t, int b, int h, int row0, int nrows, int base = 0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = threadIdx.x + NT * i;
      const int r = c / (D / 8), ch = c % (D / 8);
      if (row0 + r < nrows) {
        reg[i] = *reinterpret_cast<const bf16x8*>(t.row(b, base + row0 + r, h) + ch * 8);
      } else {
        reg[i] = bf16x8{};
      }
    }
  }
  __device__ __forceinline__ void store(unsigned char* img) const {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = threadIdx.x + NT * i;
      const int r = c / (D / 8), ch = c % (D / 8);
      *reinterpret_cast<bf16x8*>(img + lds_off<D>(r, ch)) = reg[i];
    }
  }
};

// Bias-gradient partials of a wave's 32-row output tile, without atomics: the
// column sums over the 32 rows of each lane half as a reduce-scatter (each xor
// step halves the live values: 31 shuffles for D = 64 instead of 160), then
// one plain store per value into this wave's row of a partial slab (every
// (row block, column) is written by exactly one wave; the host sums the
// slab's rows).  Lane keeps k = (lane & 31) * NV / 32 + t, k = 16 dt + r.
// m ? a : b for m = all ones / zero, one v_bfi_b32
__device__ __forceinline__ float bfi_sel(unsigned m, float a, float b) {
  float r;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
  return r;
}
template <int DT>
__device__ __forceinline__ void bias_partial(const f32x16 (&acc)[DT], float mul, float* row, int lane) {
  constexpr int NV = 16 * DT;
  float v[NV];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) v[dt * 16 + r] = acc[dt][r];
#pragma unroll
  for (int st = 0; st < 5; ++st) {
    const int o = 16 >> st, c = NV >> st;
    const unsigned m = (lane & o) ? ~0u : 0u;
#pragma unroll
    for (int i = 0; i < c / 2; ++i) {
      // bitwise selects in asm: as C selects hipcc turned the whole pass
      // into dynamically indexed array reads (cmp / cndmask chains over all
      // 32 values, 13k instructions, the kernels ran 2x slower)
      const float send = bfi_sel(m, v[i], v[i + c / 2]);
      const float keep = bfi_sel(m, v[i + c / 2], v[i]);
      v[i] = keep + __shfl_xor(send, o, 64);
    }
  }
  const int h = lane >> 5;
#pragma unroll
  for (int t = 0; t < NV / 32; ++t) {
    const int k = (lane & 31) * (NV / 32) + t, dt = k >> 4, r = k & 15;
    row[dt * 32 + acc_row(r) + 4 * h] = v[t] * mul;
  }
}

// ===========================================================================
// Forward
// DROP: the dropped probabilities are zeroed after the row sum is taken, so
// m, l and the LSE are those of the undropped softmax; the keep scale is
// folded into the epilogue's 1 / l.
// BIAS at D = 128: one wave per SIMD.  At two (256 registers, of which the
// unbiased form takes 246) the tile's 32 bias values spilled and were
// reloaded inside the tile loop (68 - 188 bytes of scratch).
template <int D, bool CAUSAL, bool DROP, bool VARLEN, bool PACKED, bool BIAS, bool GQA = false>
__global__ __launch_bounds__(256, (BIAS && D == 128 ? 1 : 2)) void attn_fwd_kernel(AttnParams P) {
  constexpr int KS = D / 16;        // k-steps over the head dim
  constexpr int DT = D / 32;        // 32-wide output tiles over the head dim
  constexpr int KV = 64;            // keys per tile
  constexpr int TILE_BYTES = KV * D * 2;
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TILE_BYTES];  // K0 V0 K1 V1

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  // causal: grid (B*H, q blocks) with the LAST (heaviest) query block of every
  // head dispatched first — longest-first order, so the kernel's tail is the
  // light blocks near the sequence start
  int bh = blockIdx.x, qb = gridDim.y - 1 - blockIdx.y;
  if (!CAUSAL) attn_head_block(bh, qb);
  const int b = bh / P.H, hh = bh % P.H;
  const int hk = kv_head<GQA>(P, hh);  // the head of every K / V address; all else stays on hh
  // packed: b is a segment; its rows are ps .. ps + plen of pack pn
  [[maybe_unused]] int pn = b, ps = 0, plen = 0;
  if constexpr (PACKED) {
    const Segment sg = segment_of(P, b);
    pn = sg.n, ps = sg.start, plen = sg.len;
  }
  const int q_blk = qb * 128;
  const int qw = q_blk + wave * 32;
  const int q = qw + (lane & 31);
  const bool q_ok = PACKED ? q < plen : q < P.Sq;  // packed: only a segment's own rows are written
  const int Skl = PACKED ? plen : key_len<VARLEN>(P, b);  // keys of this sample
  // queries of this sample: q_live rows exist, q_ok rows have an output row
  [[maybe_unused]] const int Sql = PACKED ? plen : query_len<VARLEN>(P, b);
  const bool q_live = VARLEN ? q < Sql : q_ok;
  if constexpr (VARLEN) {
    if (q_blk >= Sql) {  // a wholly dead block: o = 0, lse = -inf, no tile loop
      // packed: nothing is stored, the rows belong to the next segment or the tail
      if constexpr (!PACKED) {
        if (q_ok) {
          store_zero_rows<D>(P.o_out.row(b, q, hh), h);
          if (h == 0) P.lse[static_cast<int64_t>(bh) * P.Sq + q] = -INFINITY;
        }
      }
      return;
    }
  }

  // Q as the B operand of S^T = K Q^T: lane holds Q[q][16ks + 8h .. +8]
  bf16x8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    qf[ks] = q_live ? *reinterpret_cast<const bf16x8*>(P.q.row(pn, ps + q, hh) + ks * 16 + 8 * h) : bf16x8{};

  f32x16 o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) o[dt] = f32x16{};
  float m = -INFINITY, l = 0.f;
  // dropout: hash index of s[kt][r] = drow + k0 + kt * 32 + acc_row(r)
  [[maybe_unused]] unsigned dkey = 0, drow = 0;
  if constexpr (DROP) {
    dkey = drop_key(P, bh);
    drow = static_cast<unsigned>(q) * static_cast<unsigned>(P.Sk) + 4u * h;
  }

  int n_tiles = (Skl + KV - 1) / KV;
  if (CAUSAL) n_tiles = min(n_tiles, (q_blk + 128 + KV - 1) / KV);
  // bias: this query's row, at the lane half's first key
  [[maybe_unused]] const float* brow = nullptr;
  if constexpr (BIAS) brow = P.bias + b * P.bias_sb + hh * P.bias_sh + static_cast<int64_t>(q) * P.bias_sq + 4 * h;

  TileLoader<D, KV> kl, vl;
  kl.load(P.k, pn, hk, 0, Skl, ps);
  vl.load(P.v, pn, hk, 0, Skl, ps);
  kl.store(smem);
  vl.store(smem + TILE_BYTES);
  __syncthreads();

  // VARLEN: a wave whose 32 rows are all dead (in a block with live rows)
  // stages its share of every tile and meets the barriers, nothing else, in a
  // loop of its own: the branch is taken once, outside the tile loop below
  if constexpr (VARLEN) {
    if (__builtin_amdgcn_readfirstlane(qw) >= Sql) {
      for (int t = 0; t < n_tiles; ++t) {
        if (t + 1 < n_tiles) {
          kl.load(P.k, pn, hk, (t + 1) * KV, Skl, ps);
          vl.load(P.v, pn, hk, (t + 1) * KV, Skl, ps);
          unsigned char* nxt = smem + ((t + 1) & 1) * 2 * TILE_BYTES;
          kl.store(nxt);
          vl.store(nxt + TILE_BYTES);
        }
        __syncthreads();
      }
      n_tiles = 0;  // nothing left for the tile loop
    }
  }
  // BIAS: the bias enters as the INITIAL VALUE of the S^T accumulator,
  // S' = K Q^T + bias / scale, so that t = S' * scale_log2 = s * scale_log2 +
  // bias * log2(e): the max, the lazy-rescale test and exp2 below then work
  // on t through the code of the unbiased kernel (its "raw score" is S', the
  // biased one), and a masked key (bias = -inf) has S' = -inf like a key past
  // the sequence end.  Group kt * 4 + g of a tile holds the four keys of
  // registers 4g .. 4g + 3 of s[kt].  A tile's groups are requested at the END
  // of the tile before (here for tile 0), after that tile's P^T has been
  // consumed (the allocator still gives them 32 registers of their own, which
  // is what D = 128 pays one wave per SIMD for); they follow the K / V
  // prefetch of the same tile in issue order and precede the next one, so the
  // wait for them at the top of the tile (vmcnt retires in order) leaves the
  // prefetch issued just before it in flight.  Kept raw until then: shaping
  // them at the load would wait for the load there.
  [[maybe_unused]] f32x16 bz[BIAS ? 2 : 1];
  [[maybe_unused]] float bmul = 0.f;
  auto load_bias = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const f32x4 g = bias_group(brow, k0 + (i >> 2) * 32 + (i & 3) * 8, P.Sk - 4 * h, q_ok);
#pragma unroll
      for (int e = 0; e < 4; ++e) bz[i >> 2][(i & 3) * 4 + e] = g[e];
    }
  };
  if constexpr (BIAS) {
    bmul = P.inv_scale_log2 * kLog2e;  // 1 / scale
    load_bias(0);
  }
  for (int t = 0; t < n_tiles; ++t) {
    const int k0 = t * KV;
    const unsigned char* Kt = smem + (t & 1) * 2 * TILE_BYTES;
    const unsigned char* Vt = Kt + TILE_BYTES;
    const bool has_next = t + 1 < n_tiles;
    if (has_next) {  // issue next tile's HBM loads before this tile's MFMAs
      kl.load(P.k, pn, hk, k0 + KV, Skl, ps);
      vl.load(P.v, pn, hk, k0 + KV, Skl, ps);
    }
    const bool wave_active = !CAUSAL || (k0 <= qw + 31);
    if (wave_active) {
      // ---- S^T[key][q] for two 32-key tiles
      f32x16 s[2];
      prio_hi(P);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        s[kt] = f32x16{};
        if constexpr (BIAS) s[kt] = bz[kt] * bmul;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          bf16x8 kf = lds_read16(Kt, lds_off<D>(kt * 32 + (lane & 31), 2 * ks + h));
          s[kt] = mfma32(kf, qf[ks], s[kt]);
        }
      }
      prio_lo(P);
      // ---- mask (only tiles that cross the sequence end or the causal
      // diagonal — a wave-uniform branch), tile max of the RAW scores: the
      // softmax scale is folded into one FMA per score inside exp2 below
      const bool need_mask = (k0 + KV > Skl) || (CAUSAL && k0 + KV - 1 > qw);
      if (need_mask) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + kt * 32 + acc_row(r) + 4 * h;
            if (key >= Skl || (CAUSAL && key > q)) s[kt][r] = -INFINITY;
          }
      }
      // two independent v_max3 chains over the 32 scores (16 issues)
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
      // ---- lazy rescale: the running max m only moves when some lane's
      // tile max exceeds it by more than 8 in the log2 domain (p <= 256 is
      // exact enough in fp32 and bf16-relative); a wave-uniform branch, so
      // the o *= alpha pass runs on a few early tiles instead of every tile
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
      if constexpr (DROP) {
        const unsigned dt0 = drow + static_cast<unsigned>(k0);
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (dropped(dt0 + (kt * 32 + acc_row(r)), dkey, P.drop_thr)) s[kt][r] = 0.f;
      }
      // ---- O^T[d][q] += V^T[d][key] P^T[key][q]
      prio_hi(P);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          bf16x8 pf = acc_to_frag(s[kt], st);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            bf16x8 vf = tr_frag<D>(Vt, kt * 32 + 16 * st, dt, lane);
            o[dt] = mfma32(vf, pf, o[dt]);
          }
        }
      prio_lo(P);
    }
    if constexpr (BIAS) {
      // not to be scheduled up into the P^T V MFMAs, where s is still live
      __builtin_amdgcn_sched_barrier(0);
      if (has_next) load_bias(k0 + KV);
    }
    if (has_next) {
      unsigned char* nxt = smem + ((t + 1) & 1) * 2 * TILE_BYTES;
      kl.store(nxt);
      vl.store(nxt + TILE_BYTES);
    }
    __syncthreads();
  }

  // ---- epilogue: O = O^T / l, LSE
  float lt = l + __shfl_xor(l, 32, 64);
  if constexpr (VARLEN) {
    // a dead row of a live wave ran on Q = 0: no row sum, and a clean zero
    if (!q_live) {
      lt = 0.f;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[dt] = f32x16{};
    }
  }
  float inv = lt > 0.f ? 1.f / lt : 0.f;
  if constexpr (DROP) inv *= P.drop_rs;
  store_rows16<DT>(P.o_out.row(pn, ps + q, hh), o, inv, h, q_ok);
  // VARLEN: the LSE index is formed here from an opaque copy of the row.  The
  // dead-block exit above forms the same 64-bit index, and as one value it
  // was hoisted above the tile loop and spilled across it (non-causal D = 128
  // with dropout, 256 registers: 20 bytes of scratch and a reload in the loop)
  int ql = q;
  if constexpr (VARLEN) asm volatile("" : "+v"(ql));
  if (q_ok && h == 0)
    P.lse[stat_index<PACKED>(P, bh, pn, hh, ps + ql)] = (lt > 0.f) ? m * P.scale_log2 + log2f(lt) : -INFINITY;
}

// ===========================================================================
// dQ: query block resident (4 waves x 32 rows), loop over 64-key tiles.
//   S^T = K Q^T ; P^T = exp2(S^T*c - lse) ; dP^T = V dO^T ;
//   dS^T = P^T (dP^T - delta) ; dQ^T += K^T dS^T ; dQ = scale * dQ
// D = 64: 3 waves per SIMD (168 VGPRs) non-causal; causal needs the mask
// registers on top and spilled at 168 — a scratch reload inside the loop is a
// VMEM op, and its vmcnt wait drained the next K / V tile's prefetch every
// iteration — so the causal form runs 2 waves per SIMD without spills
// delta = rowsum(dO * O) of the block's own queries is computed here from the
// dO fragments already in registers (plus one 16-B O load per fragment) and
// written out for the dK / dV kernel, which therefore runs AFTER this one;
// there is no separate delta pass.
// DROP: dS^T = P^T (keep rs dP^T - delta); same (lane -> query, register ->
// key) coordinates as the forward.
// VARLEN with DROP (XDELTA): delta is taken from the probabilities, delta =
// sum_k P (keep rs dP), not left at dlt = rowsum(dO * O).  The two are equal
// in exact arithmetic, but O is stored in bf16 and with dropout it is rounded
// even where a row has one key (O = rs V[0]); that row's dS is exactly zero,
// and with dlt the rounding of O came out as dS instead (a sample of length 1
// put the dQ / dK error of a batch at 6e-3 to 1.1e-2 against 2.4e-3 without
// it).  Lengths make rows of few keys the normal case, so these forms pay for
// it: the loop runs on dlt as before, also sums P (keep rs dP) per lane and
// accumulates bq^T = K^T P^T from the K^T fragments of the dQ product (one
// more MFMA product, DT more accumulators), and the epilogue adds
// (dlt - delta) bq^T to dQ^T and writes delta for the dK / dV kernel.
template <int D, bool CAUSAL, bool DROP, bool VARLEN, bool PACKED, bool BIAS, bool GQA = false>
__global__ __launch_bounds__(256, (D == 64 ? (CAUSAL || DROP || BIAS ? 2 : 3) : 1)) void attn_bwd_dq_kernel(AttnParams P) {
  constexpr int KS = D / 16, DT = D / 32, KV = 64;
  constexpr int TILE_BYTES = KV * D * 2;
  constexpr bool XDELTA = VARLEN && DROP;  // delta from the probabilities (comment above)
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TILE_BYTES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  int bh = blockIdx.x, qb = gridDim.y - 1 - blockIdx.y;   // causal: longest-first (fwd)
  if (!CAUSAL) attn_head_block(bh, qb);
  const int b = bh / P.H, hh = bh % P.H;
  const int hk = kv_head<GQA>(P, hh);  // the head of every K / V address; all else stays on hh
  // packed: b is a segment; its rows are ps .. ps + plen of pack pn
  [[maybe_unused]] int pn = b, ps = 0, plen = 0;
  if constexpr (PACKED) {
    const Segment sg = segment_of(P, b);
    pn = sg.n, ps = sg.start, plen = sg.len;
  }
  const int q_blk = qb * 128;
  const int qw = q_blk + wave * 32;
  const int q = qw + (lane & 31);
  const bool q_ok = PACKED ? q < plen : q < P.Sq;  // packed: only a segment's own rows are written
  const int Skl = PACKED ? plen : key_len<VARLEN>(P, b);  // keys of this sample
  // queries of this sample: q_live rows exist, q_ok rows have a dQ row
  [[maybe_unused]] const int Sql = PACKED ? plen : query_len<VARLEN>(P, b);
  const bool q_live = VARLEN ? q < Sql : q_ok;
  if constexpr (VARLEN) {
    if (q_blk >= Sql) {  // a wholly dead block: dQ = 0 and zero dbias partials, no tile loop
      // packed: nothing is stored, the rows belong to the next segment or the tail
      if constexpr (!PACKED) {
        if (q_ok) store_zero_rows<D>(P.dq.row(b, q, hh), h);
        if (P.dbq && P.db_ld && qw < P.Sq) {
          float* drow = P.dbq + (static_cast<int64_t>(b) * ((P.Sq + 31) / 32) + qw / 32) * P.db_ld + hh * D;
          for (int c = lane; c < D; c += 64) drow[c] = 0.f;
        }
      }
      return;
    }
  }

  bf16x8 qf[KS], df[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = q_live ? *reinterpret_cast<const bf16x8*>(P.q.row(pn, ps + q, hh) + ks * 16 + 8 * h) : bf16x8{};
    df[ks] = q_live ? *reinterpret_cast<const bf16x8*>(P.dout.row(pn, ps + q, hh) + ks * 16 + 8 * h) : bf16x8{};
  }
  float lse = q_live ? P.lse[stat_index<PACKED>(P, bh, pn, hh, ps + q)] : 0.f;
  // bias: a row with every key masked has lse = -inf and t = -inf; taken as
  // +inf here, t - lse is -inf and P = 0 (not exp2(-inf + inf))
  if constexpr (BIAS) lse = (lse == -INFINITY) ? INFINITY : lse;
  [[maybe_unused]] const float* brow = nullptr;
  if constexpr (BIAS) brow = P.bias + b * P.bias_sb + hh * P.bias_sh + static_cast<int64_t>(q) * P.bias_sq + 4 * h;
  // lane (q, h) holds d = 16 ks + 8 h .. +8 of dO row q: a partial dot over
  // those, then the other half from lane ^ 32
  float part = 0.f;
  if (q_live) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 of = *reinterpret_cast<const bf16x8*>(P.o.row(pn, ps + q, hh) + ks * 16 + 8 * h);
#pragma unroll
      for (int e = 0; e < 8; ++e) part += bf2f(of[e]) * bf2f(df[ks][e]);
    }
  }
  const float dlt = part + __shfl_xor(part, 32, 64);
  if constexpr (!XDELTA)  // XDELTA writes the exact delta after the loop
    if (q_live && h == 0) P.delta[stat_index<PACKED>(P, bh, pn, hh, ps + q)] = dlt;

  f32x16 dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] = f32x16{};
  // XDELTA: bq^T = K^T P^T next to dQ^T, and this lane's share of sum_k P (keep rs dP)
  [[maybe_unused]] f32x16 bq[XDELTA ? DT : 1];
  [[maybe_unused]] float dsum = 0.f;
  if constexpr (XDELTA) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) bq[dt] = f32x16{};
  }
  [[maybe_unused]] unsigned dkey = 0, drow = 0;
  if constexpr (DROP) {
    dkey = drop_key(P, bh);
    drow = static_cast<unsigned>(q) * static_cast<unsigned>(P.Sk) + 4u * h;
  }
  // dP of register r with the dropout keep scale applied (DROP only)
  auto kept = [&](float dpv, int k0, int kt, int r) -> float {
    if constexpr (DROP) {
      const unsigned idx = drow + static_cast<unsigned>(k0) + (kt * 32 + acc_row(r));
      return dpv * (dropped(idx, dkey, P.drop_thr) ? 0.f : P.drop_rs);
    } else {
      return dpv;
    }
  };

  int n_tiles = (Skl + KV - 1) / KV;
  if (CAUSAL) n_tiles = min(n_tiles, (q_blk + 128 + KV - 1) / KV);

  TileLoader<D, KV> kl, vl;
  kl.load(P.k, pn, hk, 0, Skl, ps);
  vl.load(P.v, pn, hk, 0, Skl, ps);
  kl.store(smem);
  vl.store(smem + TILE_BYTES);
  __syncthreads();

  // VARLEN: a wholly dead wave of a live block stages tiles and meets the
  // barriers in a loop of its own (see the forward).  The tile loop is then
  // left out through its bound (D = 64) or through its start (D = 128): two
  // spellings of one thing that the register allocator tells apart.  At
  // D = 64 the bound form compiles to the allocation these kernels had before
  // they knew query lengths, and to their times; at D = 128 the causal form
  // with dropout (512 registers) reloads 7 spilled values per tile with it,
  // one more than before, and none with the start form.
  constexpr bool SKIP_BY_START = VARLEN && D == 128;
  [[maybe_unused]] int t_first = 0;
  if constexpr (VARLEN) {
    if (__builtin_amdgcn_readfirstlane(qw) >= Sql) {
      for (int t = 0; t < n_tiles; ++t) {
        if (t + 1 < n_tiles) {
          kl.load(P.k, pn, hk, (t + 1) * KV, Skl, ps);
          vl.load(P.v, pn, hk, (t + 1) * KV, Skl, ps);
          unsigned char* nxt = smem + ((t + 1) & 1) * 2 * TILE_BYTES;
          kl.store(nxt);
          vl.store(nxt + TILE_BYTES);
        }
        __syncthreads();
      }
      if constexpr (SKIP_BY_START) t_first = n_tiles;
      else n_tiles = 0;
    }
  }
  for (int t = SKIP_BY_START ? t_first : 0; t < n_tiles; ++t) {
    const int k0 = t * KV;
    const unsigned char* Kt = smem + (t & 1) * 2 * TILE_BYTES;
    const unsigned char* Vt = Kt + TILE_BYTES;
    const bool has_next = t + 1 < n_tiles;
    // bias of this tile, issued ahead of the next tile's K / V loads (see the
    // forward): group kt * 4 + g holds the keys of registers 4g .. 4g + 3
    [[maybe_unused]] f32x4 bz[BIAS ? 8 : 1];
    if constexpr (BIAS) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
        bz[i] = bias_group(brow, k0 + (i >> 2) * 32 + (i & 3) * 8, P.Sk - 4 * h, q_ok);
    }
    if (has_next) {
      kl.load(P.k, pn, hk, k0 + KV, Skl, ps);
      vl.load(P.v, pn, hk, k0 + KV, Skl, ps);
    }
    const bool wave_active = !CAUSAL || (k0 <= qw + 31);
    const bool need_mask = (k0 + KV > Skl) || (CAUSAL && k0 + KV - 1 > qw) || (qw + 31 >= (VARLEN ? Sql : P.Sq));
    if (wave_active) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        f32x16 s = f32x16{}, dp = f32x16{};
        [[maybe_unused]] bf16x8 pf[2];  // P^T as the two operand fragments (XDELTA)
        prio_hi(P);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int off = lds_off<D>(kt * 32 + (lane & 31), 2 * ks + h);
          s = mfma32(lds_read16(Kt, off), qf[ks], s);
          dp = mfma32(lds_read16(Vt, off), df[ks], dp);
        }
        prio_lo(P);
        if constexpr (BIAS) {
          // P = exp2(t - lse), t = s * scale_log2 + bias * log2(e); a masked
          // key has t = -inf and P = 0
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + kt * 32 + acc_row(r) + 4 * h;
            float pv = fexp2(fmaf(s[r], P.scale_log2, bz[kt * 4 + (r >> 2)][r & 3] * kLog2e) - lse);
            if (need_mask && (key >= Skl || !q_live)) pv = 0.f;
            s[r] = pv * (kept(dp[r], k0, kt, r) - dlt);  // dS^T
          }
        } else if (need_mask) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + kt * 32 + acc_row(r) + 4 * h;
            float pv = fexp2(s[r] * P.scale_log2 - lse);
            if (key >= Skl || (CAUSAL && key > q) || !q_live) pv = 0.f;
            if constexpr (XDELTA) {
              const float kd = kept(dp[r], k0, kt, r);
              pf[r >> 3][r & 7] = f2bf(pv);
              dsum = fmaf(pv, kd, dsum);
              s[r] = pv * (kd - dlt);
            } else {
              s[r] = pv * (kept(dp[r], k0, kt, r) - dlt);  // dS^T
            }
          }
        } else if constexpr (XDELTA) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float pv = fexp2(s[r] * P.scale_log2 - lse), kd = kept(dp[r], k0, kt, r);
            pf[r >> 3][r & 7] = f2bf(pv);
            dsum = fmaf(pv, kd, dsum);
            s[r] = pv * (kd - dlt);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) s[r] = fexp2(s[r] * P.scale_log2 - lse) * (kept(dp[r], k0, kt, r) - dlt);
        }
        prio_hi(P);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          bf16x8 sf = acc_to_frag(s, st);
          if constexpr (XDELTA) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
              const bf16x8 ktf = tr_frag<D>(Kt, kt * 32 + 16 * st, dt, lane);
              dq[dt] = mfma32(ktf, sf, dq[dt]);
              bq[dt] = mfma32(ktf, pf[st], bq[dt]);
            }
          } else {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) dq[dt] = mfma32(tr_frag<D>(Kt, kt * 32 + 16 * st, dt, lane), sf, dq[dt]);
          }
        }
        prio_lo(P);
      }
    }
    if (has_next) {
      unsigned char* nxt = smem + ((t + 1) & 1) * 2 * TILE_BYTES;
      kl.store(nxt);
      vl.store(nxt + TILE_BYTES);
    }
    __syncthreads();
  }
  if constexpr (XDELTA) {
    // dS = P (kdP - delta) = P (kdP - dlt) + P (dlt - delta): the loop used
    // dlt, the rest is one rank-1 update of dQ^T by bq^T, the query on the lane
    const float delta = dsum + __shfl_xor(dsum, 32, 64);
    const float c = dlt - delta;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[dt][r] = fmaf(c, bq[dt][r], dq[dt][r]);
    if (q_live && h == 0) P.delta[stat_index<PACKED>(P, bh, pn, hh, ps + q)] = delta;
  }
  if (P.dbq && P.db_ld) {
    if (qw < P.Sq)  // waves wholly past the sequence own no slab row
      bias_partial<DT>(dq, P.scale, P.dbq + (static_cast<int64_t>(b) * ((P.Sq + 31) / 32) + qw / 32) * P.db_ld + hh * D,
                     lane);
  } else if (P.dbq) {
    bias_colsum<DT>(dq, P.scale, P.dbq + hh * D, lane);
  }
  store_rows16<DT>(P.dq.row(pn, ps + q, hh), dq, P.scale, h, q_ok);
}

// ===========================================================================
// dK / dV: key block resident (4 waves x 32 keys), loop over 64-query tiles.
//   S = Q K^T (key on lane) ; P = exp2(S*c - lse[q]) ; dP = dO V^T ;
//   dS = P (dP - delta[q]) ; dV^T += dO^T P ; dK^T += Q^T dS ; dK = scale*dK
// DROP: the key is on the lane and the queries are in the registers, so the
// hash index q * Sk + key steps by Sk per register; the dP accumulator starts
// from zero and -delta is added after the keep scale (dS = P (keep rs dP -
// delta)); dV takes keep . P and rs at the store.
template <int D, bool CAUSAL, bool DROP, bool VARLEN, bool PACKED, bool BIAS, bool GQA = false>
__global__ __launch_bounds__(256, (D == 64 && !BIAS ? 2 : 1)) void attn_bwd_dkdv_kernel(AttnParams P) {
  constexpr int KS = D / 16, DT = D / 32, QT = 64, KW = 32;
  // prefetched LDS fragments (below): GPT causal shape 0.341 -> 0.333 ms, BERT
  // within noise (profiles/ab_attn_bwd_pf_r3.txt).  At D = 128 (one wave /
  // SIMD) the prefetch registers spill; so they do with dropout at D = 64 (256
  // registers with no room for the hash: 40 - 72 bytes of scratch, reloaded in
  // the loop): those forms take the per-pair reads
  // (BIAS holds a tile's 32 bias values in their place)
  constexpr bool PF = D == 64 && !DROP && !BIAS;
  constexpr int TILE_BYTES = QT * D * 2;
  constexpr int STAGE = 2 * TILE_BYTES + 2 * QT * 4;  // Q, dO, lse, delta
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
  // causal: heads fastest, key block 0 (the most query tiles) first — longest first
  int bh = blockIdx.x, kb = blockIdx.y;
  if (!CAUSAL) attn_head_block(bh, kb);
  // GQA: the grid runs over the B * Hkv K / V heads and hh is the K / V head
  const int b = bh / (GQA ? P.Hkv : P.H), hh = bh % (GQA ? P.Hkv : P.H);
  const int k_blk = kb * (4 * KW);
  // packed: b is a segment; its rows are ps .. ps + plen of pack pn.  Held as
  // constants (and fetch_scalars below keeps its index form per mode): as
  // mutable locals captured by the lambdas they changed the register
  // allocation of every form without packing, which are to stay the code
  // they were
  Segment sg{b, 0, 0};
  if constexpr (PACKED) sg = segment_of(P, b);
  [[maybe_unused]] const int pn = sg.n, ps = sg.start, plen = sg.len;
  // packed: a key block past the segment's end leaves here, ahead of the
  // first barrier, and stores nothing (its rows are the next segment's)
  if constexpr (PACKED) {
    if (k_blk >= plen) return;
  }
  const int kw = k_blk + wave * KW;
  // keys of this sample.  Without lengths every use reads P.Sk in place, as
  // it did before the kernel had lengths: held in a local, the causal forms
  // compiled to another instruction stream (3294 against 3305 instructions at
  // D = 64), and a call without lengths is to run the code it ran before
  [[maybe_unused]] int len_v = 0;
  if constexpr (VARLEN) len_v = PACKED ? plen : key_len<true>(P, b);
  auto Skl = [&]() -> int {
    if constexpr (VARLEN) return len_v;
    else return P.Sk;
  };
  // queries of this sample, the same way: every bound on the query axis (the
  // tile count, the tile loads, the parked -lse / c, the masks) takes it
  [[maybe_unused]] int qlen_v = 0;
  if constexpr (VARLEN) qlen_v = PACKED ? plen : query_len<true>(P, b);
  auto Sql = [&]() -> int {
    if constexpr (VARLEN) return qlen_v;
    else return P.Sq;
  };

  // K, V rows as B operands (lane holds row `key`, d = 16ks + 8h ..)
  bf16x8 kf[KS], vf[KS];
  const int key = kw + (lane & 31);
  const bool k_ok = key < Skl();                    // the key exists (VARLEN: below the sample's length)
  // the key has a dK / dV row to write: below the physical Sk; packed, only the segment's own keys
  const bool k_st = (VARLEN && !PACKED) ? key < P.Sk : k_ok;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = k_ok ? *reinterpret_cast<const bf16x8*>(P.k.row(pn, ps + key, hh) + ks * 16 + 8 * h) : bf16x8{};
    vf[ks] = k_ok ? *reinterpret_cast<const bf16x8*>(P.v.row(pn, ps + key, hh) + ks * 16 + 8 * h) : bf16x8{};
  }
  f32x16 dk[DT], dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = f32x16{};

  // VARLEN: a key block wholly past the length skips the query loop and
  // stores zeros (dK = dV = 0, and zero partials into the dbias slab); the
  // loop of a live block ends at the sample's last live query tile
  const int n_q_tiles = (VARLEN && k_blk >= Skl()) ? 0 : (Sql() + QT - 1) / QT;
  const int t0 = CAUSAL ? (k_blk / QT) : 0;
  // GQA: this workgroup serves the G query heads hh * G .. of its K / V head,
  // one after another, as ONE sequence of (head, query tile) steps: t runs
  // over t0 .. t_end, G times the tiles of a head (each head starts again at
  // t0, the key block's first causal tile), so the double buffer, the prefetch
  // and the one barrier per step carry on across the head boundaries and dK /
  // dV stay in the accumulators for the whole group.  hq / tq are the head
  // and the head's tile of step t; both are uniform over the workgroup.
  int t_end = n_q_tiles;
  [[maybe_unused]] int hq = hh, tq = t0, hq_n = hh, tq_n = t0, f_sbh = 0;
  if constexpr (GQA) {
    t_end = t0 + P.G * max(n_q_tiles - t0, 0);
    hq = hq_n = hh * P.G;
    f_sbh = b * P.H + hq;
  }
  // dropout: hash index of register r of a subtile = (first query + 4 h +
  // acc_row(r)) * Sk + key
  [[maybe_unused]] unsigned dkey = 0, dcol = 0;
  if constexpr (DROP) {
    dkey = drop_key(P, bh);
    dcol = 4u * h * static_cast<unsigned>(P.Sk) + static_cast<unsigned>(key);
  }

  TileLoader<D, QT> ql, dl;
  // row constants of a query tile, pre-shaped to seed the S and dP
  // accumulators (guide: "row constants as the initial accumulator"):
  // S' = Q K^T - lse / c, dP' = dO V^T - delta, so p = exp2(c S') and
  // dS = p dP' need no subtraction.  Fetched into registers with the tile's
  // Q / dO loads (a whole tile ahead) and parked in LDS after the compute:
  // loading them at the park point exposed one global-load latency per tile
  // to all four waves through the barrier that follows.
  // The raw values are kept until the park point and only then shaped: any
  // arithmetic on them at the fetch makes the compiler wait for the load
  // there, and vmcnt retires in order, so that wait would also drain the
  // Q / dO tile loads issued just before.
  float nls = 0.f, nds = 0.f;
  bool nok = false;
  auto fetch_scalars = [&](int q0) {
    const int qq = q0 + threadIdx.x;
    // not through Sql(): capturing that lambda here renamed two registers in
    // the causal VARLEN = false forms, which are to stay the code they were
    if constexpr (VARLEN) nok = threadIdx.x < QT && qq < qlen_v;
    else nok = threadIdx.x < QT && qq < P.Sq;
    if constexpr (PACKED) {
      if (nok) {
        nls = P.lse[stat_index<true>(P, bh, pn, hh, ps + qq)];
        nds = P.delta[stat_index<true>(P, bh, pn, hh, ps + qq)];
      }
    } else if constexpr (GQA) {
      // the rows of the query head being fetched: (b * H + hk * G + g) * Sq + q
      if (nok) {
        nls = P.lse[static_cast<int64_t>(f_sbh) * P.Sq + qq];
        nds = P.delta[static_cast<int64_t>(f_sbh) * P.Sq + qq];
      }
    } else {
      if (nok) {
        nls = P.lse[static_cast<int64_t>(bh) * P.Sq + qq];
        nds = P.delta[static_cast<int64_t>(bh) * P.Sq + qq];
      }
    }
  };
  auto park_scalars = [&](unsigned char* stage) {
    float* ls = reinterpret_cast<float*>(stage + 2 * TILE_BYTES);
    if (threadIdx.x < QT) {
      // BIAS: a row with every key masked (lse = -inf) is parked like a row
      // past Sq, S' = -inf and P = 0, not as +inf (exp2(inf - inf))
      if constexpr (BIAS) ls[threadIdx.x] = (nok && nls > -INFINITY) ? -nls * P.inv_scale_log2 : -INFINITY;
      else ls[threadIdx.x] = nok ? -nls * P.inv_scale_log2 : -INFINITY;
      ls[QT + threadIdx.x] = nok ? -nds : 0.f;
    }
  };
  // bias: the lane's key column, at the lane half's first query row; register
  // r of subtile qt is the row q0 + qt * 32 + acc_row(r) + 4 h, and the 32
  // lanes of a half read 32 consecutive keys of it (128 bytes)
  [[maybe_unused]] const float* bcol = nullptr;
  if constexpr (BIAS) bcol = P.bias + b * P.bias_sb + hh * P.bias_sh + static_cast<int64_t>(4 * h) * P.bias_sq + key;
  // unconditional (rows past Sq load as zeros without touching memory): with
  // an `if (t0 < n_q_tiles)` around it the compiler kept a CFG path from the
  // K / V fragment loads above into the loop that skipped this block's
  // vmcnt(0), so the first MFMA of EVERY iteration waited on vmcnt — and
  // vmcnt retires in order, so that wait drained the next tile's prefetch
  // right after issuing it (one exposed global-load latency per tile)
  ql.load(P.q, pn, hq, t0 * QT, Sql(), ps);
  dl.load(P.dout, pn, hq, t0 * QT, Sql(), ps);
  fetch_scalars(t0 * QT);
  ql.store(smem);
  dl.store(smem + TILE_BYTES);
  park_scalars(smem);
  __syncthreads();

  for (int t = t0; t < t_end; ++t) {
    const int q0 = (GQA ? tq : t) * QT;
    unsigned char* stage = smem + ((t - t0) & 1) * STAGE;
    const unsigned char* Qt = stage;
    const unsigned char* Dt = stage + TILE_BYTES;
    const float* ls = reinterpret_cast<const float*>(stage + 2 * TILE_BYTES);
    const float* ds = ls + QT;
    const bool has_next = t + 1 < t_end;
    // bias of this tile (bb[qt * 16 + r]), issued ahead of the next tile's
    // Q / dO loads so that the wait for it leaves that prefetch in flight
    [[maybe_unused]] float bb[BIAS ? 32 : 1];
    if constexpr (BIAS) {
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        const int rq = q0 + (i >> 4) * 32 + acc_row(i & 15);
        bb[i] = (k_ok && rq + 4 * h < P.Sq) ? bcol[static_cast<int64_t>(rq) * P.bias_sq] : 0.f;
      }
    }
    if constexpr (GQA) {
      // the next step: this head's next tile, or the first tile of the
      // group's next head (has_next: there is one)
      const bool wrap = tq + 1 == n_q_tiles;
      tq_n = wrap ? t0 : tq + 1;
      hq_n = wrap ? hq + 1 : hq;
      if (has_next) {
        f_sbh = b * P.H + hq_n;
        ql.load(P.q, pn, hq_n, tq_n * QT, Sql(), ps);
        dl.load(P.dout, pn, hq_n, tq_n * QT, Sql(), ps);
        fetch_scalars(tq_n * QT);
      }
    } else if (has_next) {
      ql.load(P.q, pn, hh, q0 + QT, Sql(), ps);
      dl.load(P.dout, pn, hh, q0 + QT, Sql(), ps);
      fetch_scalars(q0 + QT);
    }
    const bool wave_active = !CAUSAL || (q0 + QT - 1 >= kw);
    const bool need_mask = (q0 + QT > Sql()) || (CAUSAL && q0 < kw + KW - 1) || (kw + KW - 1 >= Skl());
    if (wave_active) {
      // DROP at D = 128 (all 512 registers in use): the fragment offsets of
      // the per-pair reads are derived from the lane id again in every tile.
      // As loop invariants some of them were spilled in the causal form and
      // reloaded in the loop, each reload with a vmcnt(0) wait that also
      // drains the next tile's prefetch.
      int ln = lane;
      if constexpr (DROP && D == 128) asm volatile("" : "+v"(ln));
      const int hl = ln >> 5;
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        f32x16 s, dp;
        // PF: every LDS fragment of this 32-query subtile is requested before
        // the MFMAs that consume it — the row fragments of S / dP ahead of
        // the first product, the transposed fragments of dV / dK under the
        // S / dP products and the exp2 pass — instead of one read pair per
        // MFMA pair, each waiting out the LDS latency
        [[maybe_unused]] bf16x8 qa_pf[PF ? KS : 1], da_pf[PF ? KS : 1];
        [[maybe_unused]] bf16x8 tda_pf[PF ? 2 : 1][PF ? DT : 1], tqa_pf[PF ? 2 : 1][PF ? DT : 1];
        if constexpr (PF) {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const int off = lds_off<D>(qt * 32 + (lane & 31), 2 * ks + h);
            qa_pf[ks] = lds_read16(Qt, off);
            da_pf[ks] = lds_read16(Dt, off);
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ql_ = qt * 32 + acc_row(r) + 4 * h;
          s[r] = ls[ql_];
          dp[r] = DROP ? 0.f : ds[ql_];
        }
        prio_hi(P);
        if constexpr (PF) {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            s = mfma32(qa_pf[ks], kf[ks], s);
            dp = mfma32(da_pf[ks], vf[ks], dp);
          }
#pragma unroll
          for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
              tda_pf[st][dt] = tr_frag<D>(Dt, qt * 32 + 16 * st, dt, lane);
              tqa_pf[st][dt] = tr_frag<D>(Qt, qt * 32 + 16 * st, dt, lane);
            }
        } else {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const int off = lds_off<D>(qt * 32 + (ln & 31), 2 * ks + hl);
            const bf16x8 qa = lds_read16(Qt, off), da = lds_read16(Dt, off);
            s = mfma32(qa, kf[ks], s);
            dp = mfma32(da, vf[ks], dp);
          }
        }
        prio_lo(P);
        if constexpr (DROP) {
          const unsigned dq0 = static_cast<unsigned>(q0 + qt * 32) * static_cast<unsigned>(P.Sk) + dcol;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rq = acc_row(r);
            const int qq = q0 + qt * 32 + rq + 4 * h;
            float e = s[r] * P.scale_log2;
            if constexpr (BIAS) e = fmaf(s[r], P.scale_log2, bb[qt * 16 + r] * kLog2e);
            float pv = fexp2(e);
            if (need_mask && (qq >= Sql() || (CAUSAL && key > qq) || !k_ok)) pv = 0.f;
            const bool drop = dropped(dq0 + static_cast<unsigned>(rq) * static_cast<unsigned>(P.Sk), dkey, P.drop_thr);
            dp[r] = pv * fmaf(drop ? 0.f : P.drop_rs, dp[r], ds[qt * 32 + rq + 4 * h]);
            s[r] = drop ? 0.f : pv;
          }
        } else if (need_mask) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int qq = q0 + qt * 32 + acc_row(r) + 4 * h;
            float e = s[r] * P.scale_log2;
            if constexpr (BIAS) e = fmaf(s[r], P.scale_log2, bb[qt * 16 + r] * kLog2e);
            float pv = fexp2(e);
            if (qq >= Sql() || (CAUSAL && key > qq) || !k_ok) pv = 0.f;
            s[r] = pv;
            dp[r] = pv * dp[r];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float e = s[r] * P.scale_log2;
            if constexpr (BIAS) e = fmaf(s[r], P.scale_log2, bb[qt * 16 + r] * kLog2e);
            const float pv = fexp2(e);
            s[r] = pv;
            dp[r] = pv * dp[r];
          }
        }
        prio_hi(P);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          const bf16x8 pf = acc_to_frag(s, st), sf = acc_to_frag(dp, st);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            bf16x8 da, qa;
            if constexpr (PF) {
              da = tda_pf[st][dt];
              qa = tqa_pf[st][dt];
            } else {
              da = tr_frag<D>(Dt, qt * 32 + 16 * st, dt, ln);
              qa = tr_frag<D>(Qt, qt * 32 + 16 * st, dt, ln);
            }
            dv[dt] = mfma32(da, pf, dv[dt]);
            dk[dt] = mfma32(qa, sf, dk[dt]);
          }
        }
        prio_lo(P);
      }
    }
    if (has_next) {
      unsigned char* nxt = smem + ((t + 1 - t0) & 1) * STAGE;
      ql.store(nxt);
      dl.store(nxt + TILE_BYTES);
      park_scalars(nxt);
    }
    __syncthreads();
    if constexpr (GQA) tq = tq_n, hq = hq_n;
  }
  float vmul = 1.f;  // dV's store scale: the dropout keep scale
  if constexpr (DROP) vmul = P.drop_rs;
  if (P.db_ld) {
    if (kw < P.Sk) {  // waves wholly past the sequence own no slab row
      const int64_t roff = (static_cast<int64_t>(b) * ((P.Sk + 31) / 32) + kw / 32) * P.db_ld + hh * D;
      if (P.dbk) bias_partial<DT>(dk, P.scale, P.dbk + roff, lane);
      if (P.dbv) bias_partial<DT>(dv, vmul, P.dbv + roff, lane);
    }
  } else {
    if (P.dbk) bias_colsum<DT>(dk, P.scale, P.dbk + hh * D, lane);
    if (P.dbv) bias_colsum<DT>(dv, vmul, P.dbv + hh * D, lane);
  }
  // every lane swaps; k_st guards the stores
  store_rows16<DT>(P.dk.row(pn, ps + key, hh), dk, P.scale, h, k_st);
  store_rows16<DT>(P.dv.row(pn, ps + key, hh), dv, vmul, h, k_st);
}

// ===========================================================================
// One-pass backward for D = 64, non-causal, Sk <= 512, no dbias: S, P, dP and
// dS are formed once per (query, key) tile and feed all three gradients —
// five MFMA products and one exp2 per pair instead of the seven and two of
// the dQ + dK/dV kernel pair, and Q / K / V / dO are fetched once.
//
// One workgroup (8 waves, two per SIMD) owns every key of one (batch, head)
// and walks them in at most two resident 256-key blocks.  A wave is the
// dK/dV kernel's wave: 32 keys on its lanes, dK^T / dV^T of those keys in
// registers over the whole sweep of 64-query tiles.  Added to it:
//  * dS^T crosses LDS once, as a [key][query] image of 128-byte rows (the
//    Q / K image format), double buffered; the tile's existing barrier
//    publishes it;
//  * dQ^T(tile) = K^T dS^T over the block's 256 keys, from transposed reads
//    of that image and of a K image of the block.  Four waves own the four
//    32 x 32 pieces of an even tile's dQ, the other four those of an odd
//    tile's, each one iteration behind the tile's dS: every SIMD runs the
//    same 80 MFMAs per iteration and no dQ piece is ever summed across waves;
//  * with two key blocks the first block's dQ piece goes to an fp32
//    workspace in the owning lane's own layout and the same lane adds it to
//    its piece in the second sweep: a thread re-reads only its own stores
//    (no fence, no atomics, a fixed summation order), and dQ is rounded to
//    bf16 once;
//  * delta = rowsum(dO * O) is formed from the staged dO chunk and the
//    matching O chunk while the tile is parked in LDS.
// Whole heads per workgroup: no K / V reuse across workgroups, so the grid
// needs no XCD remap.
__global__ __launch_bounds__(512, 1) void attn_bwd_onepass_kernel(AttnParams P, float* __restrict__ ws) {
  constexpr int D = 64, KS = D / 16, DT = D / 32, QT = 64, KB = 256, NT = 512;
  constexpr int TILE_BYTES = QT * D * 2;
  constexpr int STAGE = 2 * TILE_BYTES + 2 * QT * 4;  // Q, dO, -lse / c, -delta
  constexpr int KIMG_BYTES = KB * D * 2, DS_BYTES = KB * QT * 2;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE + KIMG_BYTES + 2 * DS_BYTES];
  unsigned char* const Kimg = smem + 2 * STAGE;
  unsigned char* const dSimg = Kimg + KIMG_BYTES;
  // the wave index as a scalar: what derives from it (the key block row, the
  // dQ piece, the mask test) stays out of the vector registers
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5;
  const int bh = blockIdx.x, b = bh / P.H, hh = bh % P.H;
  const int n_q_tiles = (P.Sq + QT - 1) / QT;
  const int n_kb = (P.Sk + KB - 1) / KB;
  // this wave's piece of a dQ tile it owns: queries dq_q.., columns dq_d..
  const int w4 = wave & 3, dq_par = wave >> 2, dq_q = (w4 & 1) * 32, dq_d = (w4 >> 1) * 32;
  // staging role: thread -> (row, 16-B chunk) of a 64 x 64 tile
  const int srow = threadIdx.x >> 3, sch = threadIdx.x & 7;

  TileLoader<D, QT, NT> ql, dl, ol;
  // raw values are kept until the park point (see the dK / dV kernel)
  float nls = 0.f;
  bool nok = false;
  auto fetch = [&](int q0) {
    ql.load(P.q, b, hh, q0, P.Sq);
    dl.load(P.dout, b, hh, q0, P.Sq);
    ol.load(P.o, b, hh, q0, P.Sq);
    nok = q0 + srow < P.Sq;
    if (nok && sch == 0) nls = P.lse[static_cast<int64_t>(bh) * P.Sq + q0 + srow];
  };
  auto park = [&](unsigned char* stage) {
    ql.store(stage);
    dl.store(stage + TILE_BYTES);
    float part = 0.f;  // rows past Sq loaded as zeros
#pragma unroll
    for (int e = 0; e < 8; ++e) part += bf2f(ol.reg[0][e]) * bf2f(dl.reg[0][e]);
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) part += __shfl_xor(part, o, 64);
    if (sch == 0) {
      float* ls = reinterpret_cast<float*>(stage + 2 * TILE_BYTES);
      ls[srow] = nok ? -nls * P.inv_scale_log2 : -INFINITY;
      ls[QT + srow] = -part;
    }
  };

  for (int kb = 0; kb < n_kb; ++kb) {
    const int k_blk = kb * KB;
    const int kl_ = wave * 32 + (lane & 31);  // key row inside the block
    const int kw = k_blk + wave * 32, key = k_blk + kl_;
    const bool k_ok = key < P.Sk;
    const bool last_kb = kb == n_kb - 1;
    // V rows stay in registers as B operands (lane holds row `key`, d =
    // 16 ks + 8 h ..); the K rows are re-read from the K image per subtile:
    // holding both left no room for the prefetched fragments at 256 VGPRs
    bf16x8 vf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      vf[ks] = k_ok ? *reinterpret_cast<const bf16x8*>(P.v.row(b, key, hh) + ks * 16 + 8 * h) : bf16x8{};
    }
    {
      // K image of the block: 4 rows per thread, 64 apart.  The row index is
      // made opaque so that the row pointers are formed here, per sweep: as
      // sweep invariants they were hoisted above the sweep loop and spilled
      // across the tile loop.
      int r0 = srow;
      asm volatile("" : "+v"(r0));
      const bf16* kp = P.k.row(b, k_blk + r0, hh) + sch * 8;
      bf16x8 kr[KB / 64];
#pragma unroll
      for (int i = 0; i < KB / 64; ++i)
        kr[i] = k_blk + r0 + 64 * i < P.Sk ? *reinterpret_cast<const bf16x8*>(kp + 64 * i * P.k.ss) : bf16x8{};
      int q0 = 0;  // opaque for the same reason: tile 0's fetch shares the tile loop's address form
      asm volatile("" : "+s"(q0));
      fetch(q0);
#pragma unroll
      for (int i = 0; i < KB / 64; ++i) *reinterpret_cast<bf16x8*>(Kimg + lds_off<D>(r0 + 64 * i, sch)) = kr[i];
    }
    park(smem);
    __syncthreads();

    f32x16 dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dk[dt] = dv[dt] = f32x16{};

    // dQ^T piece of tile t from the published dS^T image and the K image
    auto dq_tile = [&](int t) {
      const unsigned char* dS = dSimg + (t & 1) * DS_BYTES;
      float* wp = ws + ((static_cast<int64_t>(bh) * n_q_tiles + t) * 4 + w4) * 1024 + lane * 4;
      f32x16 acc[1] = {f32x16{}};
      // tr_frag_nat of both images, 16 keys per step: the swizzle repeats
      // every 16 rows, so a step is base + 2 KiB and the four lane offsets
      // are computed once
      const int i16 = lane & 15, colq = 16 * ((lane >> 4) & 1) + 4 * (i16 & 3), ra = 8 * h + (i16 >> 2);
      const int ck = dq_d + colq, cs = dq_q + colq;
      const unsigned char* ka = Kimg + img_off<D * 2>(ra, ck >> 3) + (ck & 7) * 2;
      const unsigned char* kb_ = Kimg + img_off<D * 2>(ra + 4, ck >> 3) + (ck & 7) * 2;
      const unsigned char* sa = dS + img_off<QT * 2>(ra, cs >> 3) + (cs & 7) * 2;
      const unsigned char* sb = dS + img_off<QT * 2>(ra + 4, cs >> 3) + (cs & 7) * 2;
      auto product = [&] {
        prio_hi(P);
#pragma unroll 4
        for (int k0 = 0; k0 < KB; k0 += 16) {
          const int o = k0 * 128;
          acc[0] = mfma32(cat44(lds_tr(ka, o), lds_tr(kb_, o)), cat44(lds_tr(sa, o), lds_tr(sb, o)), acc[0]);
        }
        prio_lo(P);
      };
      if (kb > 0) {
        // the first sweep's piece: requested ahead of the MFMAs that cover its
        // latency, added after them.  Load, product and add share one branch:
        // with the load and the add under separate tests the compiler saw a
        // path on which the load was never waited for, and made the next
        // tile's first LDS reads wait for every global load in flight, the
        // tile loads just issued among them.
        f32x4 prev[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) prev[g] = *reinterpret_cast<const f32x4*>(wp + g * 256);
        product();
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[0][4 * g + e] += prev[g][e];
      } else {
        product();
      }
      if (last_kb) {
        const int q = t * QT + dq_q + (lane & 31);
        store_rows16<1>(P.dq.row(b, q, hh) + dq_d, acc, P.scale, h, q < P.Sq);
      } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 w;
#pragma unroll
          for (int e = 0; e < 4; ++e) w[e] = acc[0][4 * g + e];
          *reinterpret_cast<f32x4*>(wp + g * 256) = w;
        }
      }
    };

    // one extra trip: dQ of a tile is formed one iteration behind its dS.  Its
    // barrier also ends the sweep: the next one overwrites the K image, stage
    // 0 and dS image 0
    for (int t = 0; t <= n_q_tiles; ++t) {
      const int q0 = t * QT;
      unsigned char* stage = smem + (t & 1) * STAGE;
      const unsigned char* Qt = stage;
      const unsigned char* Dt = stage + TILE_BYTES;
      const float* ls = reinterpret_cast<const float*>(stage + 2 * TILE_BYTES);
      const float* ds = ls + QT;
      unsigned char* dSw = dSimg + (t & 1) * DS_BYTES;
      // unconditional, like the park below (rows past Sq load as zeros
      // without touching memory): under a `has next tile` test the compiler
      // kept a path from these loads round the park's wait to the top of the
      // loop and waited there for vmcnt(0), i.e. for the dQ stores
      fetch(q0 + QT);
      const bool need_mask = (q0 + QT > P.Sq) || (kw + 31 >= P.Sk);
      if (t < n_q_tiles) {
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          // every LDS fragment of the subtile is requested ahead of the MFMAs
          // that consume it (the dK / dV kernel's PF form)
          f32x16 s, dp;
          bf16x8 qa[KS], da[KS], kf[KS], tda[2][DT], tqa[2][DT];
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            const int off = lds_off<D>(qt * 32 + (lane & 31), 2 * ks + h);
            qa[ks] = lds_read16(Qt, off);
            da[ks] = lds_read16(Dt, off);
            kf[ks] = lds_read16(Kimg, lds_off<D>(kl_, 2 * ks + h));
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int ql_ = qt * 32 + acc_row(r) + 4 * h;
            s[r] = ls[ql_];
            dp[r] = ds[ql_];
          }
          prio_hi(P);
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            s = mfma32(qa[ks], kf[ks], s);
            dp = mfma32(da[ks], vf[ks], dp);
          }
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            tda[0][dt] = tr_frag<D>(Dt, qt * 32, dt, lane);
            tqa[0][dt] = tr_frag<D>(Qt, qt * 32, dt, lane);
          }
          prio_lo(P);
          if (need_mask) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int qq = q0 + qt * 32 + acc_row(r) + 4 * h;
              float pv = fexp2(s[r] * P.scale_log2);
              if (qq >= P.Sq || !k_ok) pv = 0.f;
              s[r] = pv;
              dp[r] = pv * dp[r];
            }
          } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float pv = fexp2(s[r] * P.scale_log2);
              s[r] = pv;
              dp[r] = pv * dp[r];
            }
          }
          prio_hi(P);
#pragma unroll
          for (int st = 0; st < 2; ++st) {
            const bf16x8 pf = acc_to_frag(s, st), sf = acc_to_frag(dp, st);
            if (st == 0) {  // the second half's fragments arrive under the first half's MFMAs
#pragma unroll
              for (int dt = 0; dt < DT; ++dt) {
                tda[1][dt] = tr_frag<D>(Dt, qt * 32 + 16, dt, lane);
                tqa[1][dt] = tr_frag<D>(Qt, qt * 32 + 16, dt, lane);
              }
            }
            // dS^T[key][query]: registers 4g..4g+3 are queries 8g + 4h + 0..3
#pragma unroll
            for (int g2 = 0; g2 < 2; ++g2) {
              bf16x4 w;
#pragma unroll
              for (int e = 0; e < 4; ++e) w[e] = sf[4 * g2 + e];
              *reinterpret_cast<bf16x4*>(dSw + img_off<QT * 2>(kl_, qt * 4 + 2 * st + g2) + 8 * h) = w;
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
              dv[dt] = mfma32(tda[st][dt], pf, dv[dt]);
              dk[dt] = mfma32(tqa[st][dt], sf, dk[dt]);
            }
          }
          prio_lo(P);
        }
      }
      // park first: its wait for the tile loads would also wait out the dQ
      // stores (vmcnt counts stores), which now drain under the next tile
      park(smem + ((t + 1) & 1) * STAGE);
      if (t > 0 && ((t - 1) & 1) == dq_par) dq_tile(t - 1);
      __syncthreads();
    }

    store_rows16<DT>(P.dk.row(b, key, hh), dk, P.scale, h, k_ok);
    store_rows16<DT>(P.dv.row(b, key, hh), dv, 1.f, h, k_ok);
  }
}

// ===========================================================================
// Packed sequences: the two small kernels around the attention kernels.
//
// (start, len) of every segment from seg_lens [N, M]: one thread per pack
// scans its M slots.  start is the sum of the earlier clamped lengths, len is
// clamped to [0, min(max_seqlen, T - start)], so an over-full or negative row
// of seg_lens still describes segments inside the pack.
__global__ void attn_segment_offsets_kernel(const int32_t* __restrict__ seg_lens, int32_t* __restrict__ seg_off, int N,
                                            int M, int T, int max_seqlen) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int start = 0;
  for (int m = 0; m < M; ++m) {
    const int64_t i = static_cast<int64_t>(n) * M + m;
    const int len = min(max(seg_lens[i], 0), min(max_seqlen, T - start));
    seg_off[2 * i] = start;
    seg_off[2 * i + 1] = len;
    start += len;
  }
}

// The tail of every pack (tokens at or past the end of its last segment):
// zero rows in up to three [N, T, H, D] outputs and lse = -inf.  No attention
// workgroup writes them, and the GEMMs around attention reduce over all T rows.
// Grid (ceil(T / 16), N): a block owns 16 tokens and leaves at once when they
// are all inside segments.
__global__ __launch_bounds__(256) void attn_pack_tail_kernel(OutView a, OutView b, OutView c, float* __restrict__ lse,
                                                              const int32_t* __restrict__ seg_off, int M, int T, int H,
                                                              int D) {
  constexpr int ROWS = 16;
  const int n = blockIdx.y, row0 = blockIdx.x * ROWS;
  const int64_t last = (static_cast<int64_t>(n) * M + (M - 1)) * 2;
  const int tail = min(max(seg_off[last] + seg_off[last + 1], 0), T);
  if (row0 + ROWS <= tail) return;
  const int cpr = H * (D / 8);  // 16-byte chunks per token
  for (int i = threadIdx.x; i < ROWS * cpr; i += blockDim.x) {
    const int r = row0 + i / cpr, ch = i % cpr, hh = ch / (D / 8), d = (ch % (D / 8)) * 8;
    if (r < tail || r >= T) continue;
    const u32x4t z = {0u, 0u, 0u, 0u};
    if (a.p) *reinterpret_cast<u32x4t*>(a.row(n, r, hh) + d) = z;
    if (b.p) *reinterpret_cast<u32x4t*>(b.row(n, r, hh) + d) = z;
    if (c.p) *reinterpret_cast<u32x4t*>(c.row(n, r, hh) + d) = z;
  }
  if (lse) {
    for (int i = threadIdx.x; i < ROWS * H; i += blockDim.x) {
      const int r = row0 + i / H, hh = i % H;
      if (r >= tail && r < T) lse[(static_cast<int64_t>(n) * H + hh) * T + r] = -INFINITY;
    }
  }
}

void attention_segment_offsets(const int32_t* seg_lens, int32_t* seg_off, int N, int M, int T, int max_seqlen,
                               hipStream_t st) {
  if (N <= 0 || M <= 0 || T <= 0 || max_seqlen < 1 || max_seqlen > T)
    throw std::invalid_argument("attention: packed sequences need N, M, T > 0 and 1 <= max_seqlen <= T");
  hipLaunchKernelGGL(attn_segment_offsets_kernel, dim3(static_cast<unsigned>((N + 63) / 64)), dim3(64), 0, st,
                     seg_lens, seg_off, N, M, T, max_seqlen);
  FFK_LAUNCH_CHECK("attention_segment_offsets");
}

static void launch_pack_tail(const AttnParams& P, OutView a, OutView b, OutView c, float* lse, int N, int D,
                             hipStream_t st) {
  hipLaunchKernelGGL(attn_pack_tail_kernel, dim3(static_cast<unsigned>((P.T + 15) / 16), static_cast<unsigned>(N)),
                     dim3(256), 0, st, a, b, c, lse, P.seg_off, P.M, P.T, P.H, D);
}

// ===========================================================================
static AttnParams make_params(const AttnTensors& t, int B, int H, int Sq, int Sk, int D, float scale,
                              bool causal_grid) {
  AttnParams P{};
  auto tv = [](const AttnTensors::T& x) {
    return TensorView{static_cast<const bf16*>(x.p), x.sb, x.ss, x.sh};
  };
  auto ov = [](const AttnTensors::T& x) {
    return OutView{static_cast<bf16*>(const_cast<void*>(x.p)), x.sb, x.ss, x.sh};
  };
  P.q = tv(t.q);
  P.k = tv(t.k);
  P.v = tv(t.v);
  P.o = tv(t.o);
  P.dout = tv(t.dout);
  P.o_out = ov(t.o);
  P.dq = ov(t.dq);
  P.dk = ov(t.dk);
  P.dv = ov(t.dv);
  P.lse = t.lse;
  P.delta = t.delta;
  P.dbq = t.dbq;
  P.dbk = t.dbk;
  P.dbv = t.dbv;
  P.db_ld = t.db_ld;
  P.B = B; P.H = H; P.Sq = Sq; P.Sk = Sk;
  P.scale = scale;
  P.scale_log2 = scale * 1.4426950408889634f;
  P.inv_scale_log2 = 1.f / P.scale_log2;
  // default: on for D = 128 (forward -7 %, backward -1 %), off for D = 64
  // where it measured neutral (profiles/ab_attn_prio_r2.txt)
  static const int prio = [] {
    const char* e = getenv("FFK_ATTN_PRIO");
    return e ? atoi(e) : -1;
  }();
  P.prio = prio >= 0 ? prio : (D == 128 ? 1 : 0);
  if (t.drop_threshold) {
    if (t.drop_threshold >= (1u << 24)) throw std::invalid_argument("attention: dropout threshold must be below 2^24");
    if (static_cast<uint64_t>(Sq) * static_cast<uint64_t>(Sk) >= (1ull << 32))
      throw std::invalid_argument("attention: dropout needs Sq * Sk < 2^32");
    P.drop_thr = t.drop_threshold << 8;
    P.drop_rs = t.drop_keep_scale;
    P.seed = t.seed;
    P.seed_dev = t.seed_dev;
  }
  P.kv_lens = t.kv_lens;
  P.q_lens = t.q_lens;
  if (t.seg_offsets) {
    // packed sequences: B packs of seg_T tokens, Sq = Sk = max_seqlen
    if (t.kv_lens || t.q_lens)
      throw std::invalid_argument("attention: packed sequences (seg_lens) exclude kv_lens / q_lens");
    if (Sq != Sk)
      throw std::invalid_argument("attention: packed sequences (seg_lens) are self-attention, Sq must equal Sk");
    if (t.dbq || t.dbk || t.dbv)
      throw std::invalid_argument("attention: packed sequences (seg_lens) do not take fused dbias");
    if (t.seg_M < 1 || Sq < 1 || Sq > t.seg_T)
      throw std::invalid_argument("attention: packed sequences need M >= 1 and 1 <= max_seqlen <= T");
    if (static_cast<int64_t>(B) * t.seg_M * H > (causal_grid ? 2147483647ll : 65535ll))
      throw std::invalid_argument("attention: packed sequences: N * M * H exceeds the grid");
    P.seg_off = t.seg_offsets;
    P.M = t.seg_M;
    P.T = t.seg_T;
  }
  if (t.bias.p) {
    // the BIAS kernels exist without any other axis but dropout
    if (causal_grid) throw std::invalid_argument("attention: bias excludes causal (put the causal mask into the bias)");
    if (t.kv_lens || t.q_lens) throw std::invalid_argument("attention: bias excludes kv_lens / q_lens");
    if (t.seg_offsets) throw std::invalid_argument("attention: bias excludes packed sequences (seg_lens)");
    if (t.dbq || t.dbk || t.dbv) throw std::invalid_argument("attention: bias excludes the fused dbias");
    // one 16-byte load per four keys of a row
    if (reinterpret_cast<uintptr_t>(t.bias.p) % 16) throw std::invalid_argument("attention: bias must be 16-byte aligned");
    if (Sk % 4) throw std::invalid_argument("attention: bias needs Sk % 4 == 0");
    if (t.bias.sb % 4 || t.bias.sh % 4 || t.bias.sq % 4 || t.bias.sb < 0 || t.bias.sh < 0 || t.bias.sq < 0)
      throw std::invalid_argument("attention: bias strides must be 0 (broadcast) or positive multiples of 4");
    P.bias = t.bias.p;
    P.bias_sb = t.bias.sb;
    P.bias_sh = t.bias.sh;
    P.bias_sq = t.bias.sq;
  }
  P.Hkv = t.kv_heads > 0 ? t.kv_heads : H;
  if (t.kv_heads < 0 || H % P.Hkv)
    throw std::invalid_argument("attention: grouped-query K / V heads (kv_heads) must divide the query heads H");
  P.G = H / P.Hkv;
  if (P.G > 1) {
    // the GQA kernels exist without any other axis
    if (t.drop_threshold) throw std::invalid_argument("attention: grouped-query K / V heads (kv_heads) exclude dropout");
    if (t.kv_lens || t.q_lens)
      throw std::invalid_argument("attention: grouped-query K / V heads (kv_heads) exclude kv_lens / q_lens");
    if (t.seg_offsets)
      throw std::invalid_argument("attention: grouped-query K / V heads (kv_heads) exclude packed sequences (seg_lens)");
    if (t.bias.p) throw std::invalid_argument("attention: grouped-query K / V heads (kv_heads) exclude bias");
    if (t.dbq || t.dbk || t.dbv)
      throw std::invalid_argument("attention: grouped-query K / V heads (kv_heads) exclude the fused dbias");
  }
  return P;
}

// The runtime (D, causal) as compile-time constants: f(integral_constant<int,
// D>, bool_constant<causal>).
template <class F>
static void with_head(int D, bool causal, F&& f) {
  auto on_causal = [&](auto d) {
    if (causal) f(d, std::true_type{});
    else f(d, std::false_type{});
  };
  if (D == 64) on_causal(std::integral_constant<int, 64>{});
  else if (D == 128) on_causal(std::integral_constant<int, 128>{});
  else throw std::invalid_argument("attention: head dim must be 64 or 128");
}
// The same for (dropout, lengths): f(bool_constant<drop>, bool_constant<varlen>).
template <class F>
static void with_features(bool drop, bool varlen, F&& f) {
  auto on_varlen = [&](auto dr) {
    if (varlen) f(dr, std::true_type{});
    else f(dr, std::false_type{});
  };
  if (drop) on_varlen(std::true_type{});
  else on_varlen(std::false_type{});
}

void attention_fwd(const AttnTensors& t, int B, int H, int Sq, int Sk, int D, float scale, bool causal,
                   hipStream_t st) {
  AttnParams P = make_params(t, B, H, Sq, Sk, D, scale, causal);
  // packed: one workgroup column per segment slot, B * M * H of them
  const bool packed = P.seg_off != nullptr;
  const unsigned nq = static_cast<unsigned>((Sq + 127) / 128);
  const unsigned nbh = static_cast<unsigned>(packed ? B * P.M * H : B * H);
  dim3 grid = causal ? dim3(nbh, nq) : dim3(nq, nbh), block(256);
  with_head(D, causal, [&](auto d, auto c) {
    with_features(P.drop_thr != 0, P.kv_lens || P.q_lens || packed, [&](auto dr, auto vl) {
      constexpr int DD = decltype(d)::value;
      constexpr bool CC = decltype(c)::value, DR = decltype(dr)::value, VL = decltype(vl)::value;
      if constexpr (!DR && !VL) {
        if (P.G > 1) {  // make_params: no dropout, lengths, packing or bias
          hipLaunchKernelGGL((attn_fwd_kernel<DD, CC, false, false, false, false, true>), grid, block, 0, st, P);
          return;
        }
      }
      if constexpr (VL) {
        if (packed) {
          hipLaunchKernelGGL((attn_fwd_kernel<DD, CC, DR, true, true, false>), grid, block, 0, st, P);
          return;
        }
      }
      if constexpr (!CC && !VL) {
        if (P.bias) {
          hipLaunchKernelGGL((attn_fwd_kernel<DD, false, DR, false, false, true>), grid, block, 0, st, P);
          return;
        }
      }
      hipLaunchKernelGGL((attn_fwd_kernel<DD, CC, DR, VL, false, false>), grid, block, 0, st, P);
    });
  });
  if (packed) launch_pack_tail(P, P.o_out, OutView{}, OutView{}, P.lse, B, D, st);
  FFK_LAUNCH_CHECK("attention_fwd");
}

// The one-pass kernel's shapes.  `extras` is any of dbias, dropout and
// lengths: the kernel pair only.  The switch is read per call (the A/B tool
// and the tests flip it inside one process).
static bool onepass_eligible(int Sk, int D, bool causal, bool extras) {
  if (D != 64 || causal || Sk > 512 || extras) return false;
  const char* oe = getenv("FFK_ATTN_BWD_ONEPASS");
  return oe ? atoi(oe) != 0 : true;
}

int64_t attention_bwd_workspace(int B, int H, int Sq, int Sk, int D, bool causal, bool dbias, bool varlen) {
  if (!onepass_eligible(Sk, D, causal, dbias || varlen) || Sk <= 256) return 0;
  return static_cast<int64_t>(B) * H * ((Sq + 63) / 64) * 64 * 64;
}

int attention_bwd(const AttnTensors& t, int B, int H, int Sq, int Sk, int D, float scale, bool causal,
                  hipStream_t st, float* ws) {
  AttnParams P = make_params(t, B, H, Sq, Sk, D, scale, causal);
  const bool packed = P.seg_off != nullptr;
  const bool drop = P.drop_thr != 0, varlen = P.kv_lens || P.q_lens || packed;
  // a second key block needs the workspace: callers that pass none keep the
  // two-kernel path
  if (onepass_eligible(Sk, D, causal, t.dbq || t.dbk || t.dbv || drop || varlen || P.bias || P.G > 1) &&
      (Sk <= 256 || ws)) {
    hipLaunchKernelGGL(attn_bwd_onepass_kernel, dim3(static_cast<unsigned>(B * H)), dim3(512), 0, st, P, ws);
    FFK_LAUNCH_CHECK("attention_bwd");
    return 1;
  }
  const unsigned nq = static_cast<unsigned>((Sq + 127) / 128), nk = static_cast<unsigned>((Sk + 127) / 128);
  const unsigned nbh = static_cast<unsigned>(packed ? B * P.M * H : B * H);
  dim3 gq = causal ? dim3(nbh, nq) : dim3(nq, nbh), gk = causal ? dim3(nbh, nk) : dim3(nk, nbh), block(256);
  // dQ first: it writes the delta that the dK / dV kernel reads
  with_head(D, causal, [&](auto d, auto c) {
    with_features(drop, varlen, [&](auto dr, auto vl) {
      constexpr int DD = decltype(d)::value;
      constexpr bool CC = decltype(c)::value, DR = decltype(dr)::value, VL = decltype(vl)::value;
      if constexpr (!DR && !VL) {
        if (P.G > 1) {
          // dQ over the B * H query heads, dK/dV over the B * Hkv K / V heads
          const unsigned nkh = static_cast<unsigned>(B * P.Hkv);
          const dim3 gkv = causal ? dim3(nkh, nk) : dim3(nk, nkh);
          hipLaunchKernelGGL((attn_bwd_dq_kernel<DD, CC, false, false, false, false, true>), gq, block, 0, st, P);
          hipLaunchKernelGGL((attn_bwd_dkdv_kernel<DD, CC, false, false, false, false, true>), gkv, block, 0, st, P);
          return;
        }
      }
      if constexpr (VL) {
        if (packed) {
          hipLaunchKernelGGL((attn_bwd_dq_kernel<DD, CC, DR, true, true, false>), gq, block, 0, st, P);
          hipLaunchKernelGGL((attn_bwd_dkdv_kernel<DD, CC, DR, true, true, false>), gk, block, 0, st, P);
          return;
        }
      }
      if constexpr (!CC && !VL) {
        if (P.bias) {
          hipLaunchKernelGGL((attn_bwd_dq_kernel<DD, false, DR, false, false, true>), gq, block, 0, st, P);
          hipLaunchKernelGGL((attn_bwd_dkdv_kernel<DD, false, DR, false, false, true>), gk, block, 0, st, P);
          return;
        }
      }
      hipLaunchKernelGGL((attn_bwd_dq_kernel<DD, CC, DR, VL, false, false>), gq, block, 0, st, P);
      hipLaunchKernelGGL((attn_bwd_dkdv_kernel<DD, CC, DR, VL, false, false>), gk, block, 0, st, P);
    });
  });
  if (packed) launch_pack_tail(P, P.dq, P.dk, P.dv, nullptr, B, D, st);
  FFK_LAUNCH_CHECK("attention_bwd");
  return 0;
}

}  // namespace ffk
