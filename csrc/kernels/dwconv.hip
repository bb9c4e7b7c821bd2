// Depthwise convolution (groups == C == K) for gfx950: direct stencil kernels,
// NHWC activations (bf16 or fp32), weight [C][R][S], fp32 arithmetic.
//
// A depthwise convolution contracts over R * S taps only, so there is nothing
// for a matrix instruction to do: it reads x once, writes y once and does
// R * S multiply-adds per element.  The kernels here are built for that.
//
// Common tiling.  A workgroup of 256 threads owns a 64-channel slice.  A thread
// holds one 16-byte channel vector (V = 8 bf16 or 4 fp32 channels): CL = 64 / V
// channel lanes (8 or 16) times PT = 256 / CL pixel threads (32 or 16).  Global
// and LDS accesses are 16 bytes wide; 16 consecutive lanes read 256 contiguous
// LDS bytes (2 bf16 pixels next to each other along q, or 1 fp32 pixel), so the
// patch reads are conflict-free across the channel lanes at stride 1 (2-way at
// stride 2 in bf16, where the pixels of a lane group lie 256 bytes apart).
// Pixel offsets in global memory are 64-bit.
//
//   * dw_tile_kernel<T, NPIX, false> (forward): the pixel threads form a
//     tpt x tqt grid and each owns NPIX output rows (tile TP x TQ = tpt * NPIX x
//     tqt, 16 x 8 for bf16, 8 x 8 for fp32).  The input patch
//     ((TP-1) sh + (R-1) dh + 1) x ((TQ-1) sw + (S-1) dw + 1) x 64 channels is
//     staged into LDS in the input type with out-of-image and out-of-channel
//     positions as zeros, the slice's filters transposed into LDS as fp32
//     [R*S][64].  Per tap a thread reads its V weights once (an LDS broadcast
//     over the pixel threads) and NPIX patch vectors: NPIX * V FMAs for
//     NPIX + V / 4 LDS reads, no bounds tests.  Epilogue: bias, activation, one
//     rounding, 16-byte stores, guarded at the channel and pixel tails.
//   * dw_tile_kernel<T, NPIX, true> (dgrad): the same body tiled over dx pixels
//     as a gather.  The dy patch (floor((TP-1 + (R-1) dh) / sh) + 1 rows) is
//     staged the same way, plus one all-zero pixel.  Which dy row a (dx row,
//     r) pair reads -- or none, when (h + ph - r dh) % sh != 0 -- is worked out
//     once per workgroup into two small LDS tables (rows x R, columns x S), so
//     the inner loop has no division and no branch: a tap with no contribution
//     reads the zero pixel.  One body serves every stride; a stride-1
//     specialisation was not written (nothing measured asks for it).  dx pixels
//     that no output touches come out as beta * dx, exactly 0 at beta = 0.
//   * The launch code takes the first tile of a fixed list whose LDS need is
//     at most 60 KiB (NPIX 4 -> 2 -> 1, then smaller thread grids with idle
//     pixel threads, down to 1 x 1), starting lower for images of at most 8 / 4
//     rows.  The choice depends on the shape and type only.
//   * dw_wgrad_kernel: grid = (64-channel slice, chunk of consecutive output
//     tiles in (n, p-tile, q-tile) order).  Per tile the workgroup stages the dy
//     tile (zeros past P / Q) and the matching x patch, then works through
//     R*S * NS units (tap, pixel stripe), NS = min(8, 64 / (R*S)): a pixel
//     thread takes units pt, pt + PT, ..; per unit it sums dy * x over the
//     stripe's pixels in registers and adds the V sums into its own fp32 slot of
//     an LDS accumulator [R*S * NS][64] (one owner per slot: no race, fixed
//     order).  After the chunk's last tile the stripes are summed in index order
//     and written to ws[chunk][R*S][C].  dw_wgrad_reduce_kernel adds the chunks
//     in index order into dw[c][r][s].  No atomics; the chunk count is a
//     function of the shape alone (about 2048 workgroups, at least 4 tiles per
//     chunk), so results are bit-reproducible.
//
// Deviations from the first sketch of this design: the forward's fp32 tile is
// 8 x 8 (2 x 8 pixel threads) rather than 16 x 4, the weight gradient tiles
// (n, p, q) rather than whole (n, p) rows (a 7-row x patch of a 112-wide image
// does not fit in LDS), and tap / stripe sums live in LDS rather than in
// registers (R * S up to 49 sums per lane would be indexed at run time).
// Measured (profiles/dwconv.txt): forward and dgrad beat the super-group MFMA
// path at every shape tried; the bf16 weight gradient does not (two barriers
// and an LDS read-modify-write of the tap sums per 64-pixel tile), so
// ops/conv.py sends most bf16 weight gradients to conv2d_grouped_wgrad.
// Dilations so large that a single output pixel's footprint does not fit in
// 60 KiB of LDS are refused by dwconv_supported.
#include "common.h"
#include "kernels.h"

namespace ffk {

namespace {

constexpr int NT = 256;
constexpr int CS = 64;             // channels per workgroup
constexpr int LDS_MAX = 60 * 1024;   // dynamic part; the static tables ride on top, 64 KiB in all
constexpr int MAX_TP = 16, MAX_TQ = 8, MAX_F = 7;

template <class T>
struct Tr;
template <>
struct Tr<bf16> {
  typedef bf16x8 vec;
  static constexpr int V = 8;
};
template <>
struct Tr<float> {
  typedef f32x4 vec;
  static constexpr int V = 4;
};

template <int ACT, int N>
__device__ __forceinline__ void apply_act(float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = act_ct<ACT>(v[i]);
}

__host__ __device__ inline int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
__host__ __device__ inline int ceil_div(int a, int b) { return floor_div(a + b - 1, b); }

struct DwArgs {
  const void* in;     // forward: x; dgrad: dy
  const void* w;      // [C][R][S]
  const void* bias;   // forward only, may be null
  void* out;          // forward: y; dgrad: dx
  int N, IH, IW;      // extent of the staged tensor
  int OH, OW;         // extent of the tiled tensor
  int C, R, S, sh, sw, ph, pw, dh, dw;
  int tpt, tqt;       // pixel-thread grid, tpt * tqt <= PT
  int PH, PW;         // staged patch
  int tiles_p, tiles_q, cslices;
  int act;
  float beta;
};

// Patch pixel i (row-major PH x PW, origin (i0, j0) in the staged tensor) ->
// LDS, zeros outside the tensor and past the last channel.
template <class T>
__device__ __forceinline__ void stage_patch(typename Tr<T>::vec* patch, const T* in, int64_t n, int IH, int IW, int C,
                                            int c, int i0, int j0, int PH, int PW) {
  using vec = typename Tr<T>::vec;
  constexpr int CL = CS / Tr<T>::V, PT = NT / CL;
  const int cl = threadIdx.x % CL;
  const int npx = PH * PW;
  for (int i = threadIdx.x / CL; i < npx; i += PT) {
    const int pr = i / PW, pc = i - pr * PW;
    const int ih = i0 + pr, iw = j0 + pc;
    vec v = vec{};
    if (c < C && ih >= 0 && ih < IH && iw >= 0 && iw < IW)
      v = *reinterpret_cast<const vec*>(in + ((n * IH + ih) * IW + iw) * C + c);
    patch[i * CL + cl] = v;
  }
}

template <class T, int NPIX, bool DGRAD>
__global__ __launch_bounds__(NT) void dw_tile_kernel(DwArgs a) {
  using vec = typename Tr<T>::vec;
  constexpr int V = Tr<T>::V, CL = CS / V;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int rtab[MAX_TP * MAX_F], ctab[MAX_TQ * MAX_F];
  const int RS = a.R * a.S;
  float* wl = reinterpret_cast<float*>(smem);                 // [RS][64]
  vec* patch = reinterpret_cast<vec*>(smem + RS * CS * 4);     // [PH * PW + 1][CL]

  unsigned b = blockIdx.x;
  const int c0 = static_cast<int>(b % a.cslices) * CS;
  b /= a.cslices;
  const int tq_i = b % a.tiles_q;
  b /= a.tiles_q;
  const int tp_i = b % a.tiles_p;
  const int64_t n = b / a.tiles_p;
  const int TP = a.tpt * NPIX, TQ = a.tqt;
  const int o0 = tp_i * TP, o1 = tq_i * TQ;
  const int i0 = DGRAD ? ceil_div(o0 + a.ph - (a.R - 1) * a.dh, a.sh) : o0 * a.sh - a.ph;
  const int j0 = DGRAD ? ceil_div(o1 + a.pw - (a.S - 1) * a.dw, a.sw) : o1 * a.sw - a.pw;

  const int cl = threadIdx.x % CL, pt = threadIdx.x / CL;
  const int c = c0 + cl * V;
  const int npx = a.PH * a.PW;

  // filters of the slice, transposed: wl[t][c]
  const T* w = static_cast<const T*>(a.w);
  for (int i = threadIdx.x; i < RS * CS; i += NT) {
    const int ch = i / RS, t = i - ch * RS;
    wl[t * CS + ch] = c0 + ch < a.C ? static_cast<float>(w[static_cast<int64_t>(c0 + ch) * RS + t]) : 0.f;
  }
  stage_patch<T>(patch, static_cast<const T*>(a.in), n, a.IH, a.IW, a.C, c, i0, j0, a.PH, a.PW);
  if (DGRAD) {
    if (pt == 0) patch[npx * CL + cl] = vec{};
    // dx row o0 + hl and tap r read dy row (h + ph - r dh) / sh when that divides
    for (int i = threadIdx.x; i < TP * a.R; i += NT) {
      const int hl = i / a.R, r = i - hl * a.R;
      const int hh = o0 + hl + a.ph - r * a.dh;
      const int row = hh / a.sh - i0;
      rtab[i] = (hh % a.sh == 0 && row >= 0 && row < a.PH) ? row : -1;
    }
    for (int i = threadIdx.x; i < TQ * a.S; i += NT) {
      const int wl_ = i / a.S, s = i - wl_ * a.S;
      const int ww = o1 + wl_ + a.pw - s * a.dw;
      const int col = ww / a.sw - j0;
      ctab[i] = (ww % a.sw == 0 && col >= 0 && col < a.PW) ? col : -1;
    }
  }
  __syncthreads();
  if (pt >= a.tpt * a.tqt) return;   // idle pixel threads of a reduced tile

  const int tq = pt % a.tqt, tp = pt / a.tqt;
  float acc[NPIX][V];
#pragma unroll
  for (int j = 0; j < NPIX; ++j)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[j][v] = 0.f;

  for (int r = 0; r < a.R; ++r) {
    int row[NPIX];
#pragma unroll
    for (int j = 0; j < NPIX; ++j) {
      const int pl = j * a.tpt + tp;
      row[j] = DGRAD ? rtab[pl * a.R + r] : pl * a.sh + r * a.dh;
    }
    for (int s = 0; s < a.S; ++s) {
      const int col = DGRAD ? ctab[tq * a.S + s] : tq * a.sw + s * a.dw;
      float wv[V];
      const float* wp = wl + (r * a.S + s) * CS + cl * V;
#pragma unroll
      for (int v4 = 0; v4 < V; v4 += 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(wp + v4);
#pragma unroll
        for (int e = 0; e < 4; ++e) wv[v4 + e] = t[e];
      }
#pragma unroll
      for (int j = 0; j < NPIX; ++j) {
        int off = row[j] * a.PW + col;
        if (DGRAD) off = (row[j] < 0 || col < 0) ? npx : off;
        const vec xv = patch[off * CL + cl];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[j][v] = __builtin_fmaf(static_cast<float>(xv[v]), wv[v], acc[j][v]);
      }
    }
  }

  const int oc = o1 + tq;
  if (c >= a.C || oc >= a.OW) return;
  float bv[V];
#pragma unroll
  for (int v = 0; v < V; ++v) bv[v] = 0.f;
  if (!DGRAD && a.bias) {
    const vec t = *reinterpret_cast<const vec*>(static_cast<const T*>(a.bias) + c);
#pragma unroll
    for (int v = 0; v < V; ++v) bv[v] = static_cast<float>(t[v]);
  }
  T* out = static_cast<T*>(a.out);
#pragma unroll
  for (int j = 0; j < NPIX; ++j) {
    const int orow = o0 + j * a.tpt + tp;
    if (orow >= a.OH) continue;
    T* dst = out + ((n * a.OH + orow) * a.OW + oc) * a.C + c;
    if (DGRAD) {
      if (a.beta != 0.f) {
        const vec old = *reinterpret_cast<const vec*>(dst);
#pragma unroll
        for (int v = 0; v < V; ++v) acc[j][v] = __builtin_fmaf(a.beta, static_cast<float>(old[v]), acc[j][v]);
      }
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v) acc[j][v] += bv[v];
      switch (a.act) {
        case 1: apply_act<1>(acc[j]); break;
        case 2: apply_act<2>(acc[j]); break;
        case 3: apply_act<3>(acc[j]); break;
        default: break;
      }
    }
    vec o;
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = static_cast<T>(acc[j][v]);
    *reinterpret_cast<vec*>(dst) = o;
  }
}

struct DwWgradArgs {
  const void* x;
  const void* dy;
  float* ws;   // [chunks][R*S][C]
  int N, H, W, P, Q, C, R, S, sh, sw, ph, pw, dh, dw;
  int TP, lq;        // tile TP x (1 << lq)
  int PH, PW, NS;    // x patch, pixel stripes per tap
  int tiles_p, tiles_q, cslices;
  int64_t ntiles;
  int tiles_per_chunk;
};

template <class T>
__global__ __launch_bounds__(NT) void dw_wgrad_kernel(DwWgradArgs a) {
  using vec = typename Tr<T>::vec;
  constexpr int V = Tr<T>::V, CL = CS / V, PT = NT / CL;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int ubase[CS], ustripe[CS];   // per unit: patch offset of its tap, its stripe
  const int RS = a.R * a.S, units = RS * a.NS;
  const int TQ = 1 << a.lq, tpx = a.TP * TQ;
  float* lacc = reinterpret_cast<float*>(smem);                          // [units][64]
  vec* dyt = reinterpret_cast<vec*>(smem + units * CS * 4);              // [tpx][CL]
  vec* xp = dyt + tpx * CL;                                              // [PH * PW][CL]

  const int c0 = static_cast<int>(blockIdx.x % a.cslices) * CS;
  const int64_t chunk = blockIdx.x / a.cslices;
  const int cl = threadIdx.x % CL, pt = threadIdx.x / CL;
  const int c = c0 + cl * V;

  for (int i = threadIdx.x; i < units * CS; i += NT) lacc[i] = 0.f;
  for (int u = threadIdx.x; u < units; u += NT) {
    const int t = u / a.NS, r = t / a.S, s = t - r * a.S;
    ubase[u] = r * a.dh * a.PW + s * a.dw;
    ustripe[u] = u - t * a.NS;
  }

  const T* x = static_cast<const T*>(a.x);
  const T* dy = static_cast<const T*>(a.dy);
  const int64_t t0 = chunk * a.tiles_per_chunk;
  const int64_t t1 = t0 + a.tiles_per_chunk < a.ntiles ? t0 + a.tiles_per_chunk : a.ntiles;
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int tq_i = static_cast<int>(tile % a.tiles_q);
    const int64_t rest = tile / a.tiles_q;
    const int tp_i = static_cast<int>(rest % a.tiles_p);
    const int64_t n = rest / a.tiles_p;
    const int o0 = tp_i * a.TP, o1 = tq_i * TQ;
    __syncthreads();   // the previous tile's reads are done (first pass: lacc and the unit tables are written)
    for (int i = pt; i < tpx; i += PT) {
      const int p = o0 + (i >> a.lq), q = o1 + (i & (TQ - 1));
      vec v = vec{};
      if (c < a.C && p < a.P && q < a.Q) v = *reinterpret_cast<const vec*>(dy + ((n * a.P + p) * a.Q + q) * a.C + c);
      dyt[i * CL + cl] = v;
    }
    stage_patch<T>(xp, x, n, a.H, a.W, a.C, c, o0 * a.sh - a.ph, o1 * a.sw - a.pw, a.PH, a.PW);
    __syncthreads();
    for (int u = pt; u < units; u += PT) {
      const int base = ubase[u];
      float acc[V];
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = 0.f;
#pragma unroll 4   // independent LDS reads in flight: the sum is a short dependent chain otherwise
      for (int pix = ustripe[u]; pix < tpx; pix += a.NS) {
        const int off = (pix >> a.lq) * a.sh * a.PW + (pix & (TQ - 1)) * a.sw + base;
        const vec d = dyt[pix * CL + cl];
        const vec xv = xp[off * CL + cl];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = __builtin_fmaf(static_cast<float>(d[v]), static_cast<float>(xv[v]), acc[v]);
      }
      float* slot = lacc + u * CS + cl * V;   // owned by this thread alone
#pragma unroll
      for (int v4 = 0; v4 < V; v4 += 4) {
        f32x4 t = *reinterpret_cast<f32x4*>(slot + v4);
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] += acc[v4 + e];
        *reinterpret_cast<f32x4*>(slot + v4) = t;
      }
    }
  }
  __syncthreads();
  // stripes summed in index order -> ws[chunk][t][c]
  for (int i = threadIdx.x; i < RS * CS; i += NT) {
    const int t = i / CS, ch = i - t * CS;
    float sum = 0.f;
    for (int s = 0; s < a.NS; ++s) sum += lacc[(t * a.NS + s) * CS + ch];
    if (c0 + ch < a.C) a.ws[(chunk * RS + t) * a.C + c0 + ch] = sum;
  }
}

// dw[c][t] += sum over chunks (index order) of ws[chunk][t][c]
__global__ __launch_bounds__(NT) void dw_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                             int chunks, int RS, int C) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= RS * C) return;
  const int t = i / C, c = i - t * C;
  float sum = 0.f;
  for (int k = 0; k < chunks; ++k) sum += ws[(static_cast<int64_t>(k) * RS + t) * C + c];
  dw[static_cast<int64_t>(c) * RS + t] += sum;
}

// ---------------------------------------------------------------------------
// host side: tile plans (functions of the shape and the type only)
inline int out_dim(int in, int pad, int dil, int f, int stride) { return (in + 2 * pad - dil * (f - 1) - 1) / stride + 1; }

struct TilePlan {
  int npix = 0, tpt = 0, tqt = 0, PH = 0, PW = 0;
  size_t lds = 0;
  bool ok = false;
};

// forward (dgrad = false: tiles of y, patch of x) or dgrad (tiles of dx, patch of dy)
TilePlan tile_plan(const ConvShape& s, int dtype, bool dgrad) {
  static const int bf[][3] = {{4, 4, 8}, {2, 4, 8}, {1, 4, 8}, {1, 4, 4}, {1, 2, 4}, {1, 2, 2}, {1, 1, 2}, {1, 1, 1}};
  static const int f32[][3] = {{4, 2, 8}, {2, 2, 8}, {1, 2, 8}, {1, 2, 4}, {1, 2, 2}, {1, 1, 2}, {1, 1, 1}, {1, 1, 1}};
  const int (*cand)[3] = dtype == kBF16 ? bf : f32;
  const int esz = dtype == kBF16 ? 2 : 4;
  const int rows = dgrad ? s.H : out_dim(s.H, s.ph, s.dh, s.R, s.sh);
  // short images start at a shorter tile: fewer idle rows
  const int first = rows * 2 > cand[0][0] * cand[0][1] ? 0 : (rows * 2 > cand[1][0] * cand[1][1] ? 1 : 2);
  TilePlan p;
  for (int i = first; i < 8; ++i) {
    const int TP = cand[i][0] * cand[i][1], TQ = cand[i][2];
    const int PH = dgrad ? (TP - 1 + (s.R - 1) * s.dh) / s.sh + 1 : (TP - 1) * s.sh + (s.R - 1) * s.dh + 1;
    const int PW = dgrad ? (TQ - 1 + (s.S - 1) * s.dw) / s.sw + 1 : (TQ - 1) * s.sw + (s.S - 1) * s.dw + 1;
    const size_t lds = static_cast<size_t>(s.R) * s.S * CS * 4 + (static_cast<size_t>(PH) * PW + 1) * CS * esz;
    if (lds <= LDS_MAX) {
      p.npix = cand[i][0], p.tpt = cand[i][1], p.tqt = TQ, p.PH = PH, p.PW = PW, p.lds = lds, p.ok = true;
      return p;
    }
  }
  return p;
}

struct WgradPlan {
  int TP = 0, lq = 0, PH = 0, PW = 0, NS = 0, tiles_p = 0, tiles_q = 0, cslices = 0, tiles_per_chunk = 0;
  int64_t ntiles = 0, chunks = 0;
  size_t lds = 0;
  bool ok = false;
};

WgradPlan wgrad_plan(const ConvShape& s, int dtype) {
  static const int cand[][2] = {{8, 3}, {4, 3}, {4, 2}, {2, 2}, {2, 1}, {1, 1}, {1, 0}};
  const int esz = dtype == kBF16 ? 2 : 4;
  const int P = out_dim(s.H, s.ph, s.dh, s.R, s.sh), Q = out_dim(s.W, s.pw, s.dw, s.S, s.sw);
  const int RS = s.R * s.S;
  WgradPlan p;
  p.NS = CS / RS < 1 ? 1 : (CS / RS > 8 ? 8 : CS / RS);
  for (const auto& cd : cand) {
    const int TP = cd[0], TQ = 1 << cd[1];
    const int PH = (TP - 1) * s.sh + (s.R - 1) * s.dh + 1, PW = (TQ - 1) * s.sw + (s.S - 1) * s.dw + 1;
    const size_t lds = static_cast<size_t>(RS) * p.NS * CS * 4 + static_cast<size_t>(TP) * TQ * CS * esz +
                       static_cast<size_t>(PH) * PW * CS * esz;
    if (lds > LDS_MAX) continue;
    p.TP = TP, p.lq = cd[1], p.PH = PH, p.PW = PW, p.lds = lds, p.ok = true;
    p.tiles_p = (P + TP - 1) / TP, p.tiles_q = (Q + TQ - 1) / TQ, p.cslices = (s.C + CS - 1) / CS;
    p.ntiles = static_cast<int64_t>(s.N) * p.tiles_p * p.tiles_q;
    // about 2048 workgroups, at least 4 tiles per chunk
    int64_t chunks = (2048 + p.cslices - 1) / p.cslices;
    if (chunks > (p.ntiles + 3) / 4) chunks = (p.ntiles + 3) / 4;
    if (chunks < 1) chunks = 1;
    const int64_t per = (p.ntiles + chunks - 1) / chunks;
    p.tiles_per_chunk = static_cast<int>(per);
    p.chunks = (p.ntiles + per - 1) / per;
    return p;
  }
  return p;
}

bool shape_ok(const ConvShape& s) {
  if (s.N <= 0 || s.H <= 0 || s.W <= 0 || s.C <= 0 || s.C != s.K) return false;
  if (s.R < 1 || s.R > MAX_F || s.S < 1 || s.S > MAX_F) return false;
  if (s.sh < 1 || s.sw < 1 || s.dh < 1 || s.dw < 1 || s.ph < 0 || s.pw < 0) return false;
  // geometry terms stay far inside 31 bits
  for (int v : {s.H, s.W, s.sh, s.sw, s.dh, s.dw, s.ph, s.pw})
    if (v > (1 << 24)) return false;
  if (static_cast<int64_t>(s.H) + 2 * s.ph < static_cast<int64_t>(s.dh) * (s.R - 1) + 1) return false;
  if (static_cast<int64_t>(s.W) + 2 * s.pw < static_cast<int64_t>(s.dw) * (s.S - 1) + 1) return false;
  return true;
}

void require(const char* who, const ConvShape& s, int dtype, std::initializer_list<const void*> ps) {
  const std::string w(who);
  if (!dwconv_supported(s, dtype))
    throw std::invalid_argument(w + ": needs groups == C == K, bf16 with C % 8 == 0 or fp32 with C % 4 == 0, "
                                    "filters of 1..7, and a geometry whose smallest tile fits in LDS");
  uintptr_t bits = 0;
  for (const void* p : ps) {
    if (!p) throw std::invalid_argument(w + ": missing operand");
    bits |= reinterpret_cast<uintptr_t>(p);
  }
  if (bits & 15) throw std::invalid_argument(w + ": operands must be 16-byte aligned");
}

template <class T, bool DGRAD>
void launch_tile(const TilePlan& p, const DwArgs& a, unsigned blocks, hipStream_t st) {
  auto k = p.npix == 4 ? dw_tile_kernel<T, 4, DGRAD> : (p.npix == 2 ? dw_tile_kernel<T, 2, DGRAD>
                                                                    : dw_tile_kernel<T, 1, DGRAD>);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(NT), p.lds, st, a);
}

void run_tile(const char* who, bool dgrad, int dtype, const ConvShape& s, DwArgs a, hipStream_t st) {
  const TilePlan p = tile_plan(s, dtype, dgrad);
  a.N = s.N, a.C = s.C, a.R = s.R, a.S = s.S;
  a.sh = s.sh, a.sw = s.sw, a.ph = s.ph, a.pw = s.pw, a.dh = s.dh, a.dw = s.dw;
  const int P = out_dim(s.H, s.ph, s.dh, s.R, s.sh), Q = out_dim(s.W, s.pw, s.dw, s.S, s.sw);
  a.IH = dgrad ? P : s.H, a.IW = dgrad ? Q : s.W;
  a.OH = dgrad ? s.H : P, a.OW = dgrad ? s.W : Q;
  a.tpt = p.tpt, a.tqt = p.tqt, a.PH = p.PH, a.PW = p.PW;
  const int TP = p.tpt * p.npix;
  a.tiles_p = (a.OH + TP - 1) / TP, a.tiles_q = (a.OW + p.tqt - 1) / p.tqt, a.cslices = (s.C + CS - 1) / CS;
  const int64_t blocks = static_cast<int64_t>(s.N) * a.tiles_p * a.tiles_q * a.cslices;
  if (blocks >= (int64_t(1) << 31)) throw std::invalid_argument(std::string(who) + ": grid too large");
  const unsigned nb = static_cast<unsigned>(blocks);
  if (dtype == kBF16)
    dgrad ? launch_tile<bf16, true>(p, a, nb, st) : launch_tile<bf16, false>(p, a, nb, st);
  else
    dgrad ? launch_tile<float, true>(p, a, nb, st) : launch_tile<float, false>(p, a, nb, st);
  FFK_LAUNCH_CHECK(who);
}

}  // namespace

bool dwconv_supported(const ConvShape& s, int dtype) {
  if (dtype != kBF16 && dtype != kF32) return false;
  if (!shape_ok(s)) return false;
  if (s.C % (dtype == kBF16 ? 8 : 4)) return false;
  return tile_plan(s, dtype, false).ok && tile_plan(s, dtype, true).ok && wgrad_plan(s, dtype).ok;
}

void dwconv_fwd(int dtype, const ConvShape& s, const void* x, const void* w, const void* bias, void* y, int act,
                hipStream_t st) {
  require("dwconv_fwd", s, dtype, {x, w, y});
  if (act < 0 || act > 3) throw std::invalid_argument("dwconv_fwd: activation must be none / relu / sigmoid / tanh");
  if (reinterpret_cast<uintptr_t>(bias) & 15) throw std::invalid_argument("dwconv_fwd: bias must be 16-byte aligned");
  DwArgs a{};
  a.in = x, a.w = w, a.bias = bias, a.out = y, a.act = act, a.beta = 0.f;
  run_tile("dwconv_fwd", false, dtype, s, a, st);
}

void dwconv_dgrad(int dtype, const ConvShape& s, const void* dy, const void* w, void* dx, float beta,
                  hipStream_t st) {
  require("dwconv_dgrad", s, dtype, {dy, w, dx});
  DwArgs a{};
  a.in = dy, a.w = w, a.bias = nullptr, a.out = dx, a.act = 0, a.beta = beta;
  run_tile("dwconv_dgrad", true, dtype, s, a, st);
}

int64_t dwconv_wgrad_ws_floats(const ConvShape& s) {
  if (!shape_ok(s)) throw std::invalid_argument("dwconv_wgrad_ws_floats: not a depthwise shape this file serves");
  // the type is not known here: the larger of the two plans
  const WgradPlan a = wgrad_plan(s, kBF16), b = wgrad_plan(s, kF32);
  const int64_t chunks = a.chunks > b.chunks ? a.chunks : b.chunks;
  return chunks * s.R * s.S * s.C;
}

void dwconv_wgrad(int dtype, const ConvShape& s, const void* x, const void* dy, float* dw, float* ws,
                  hipStream_t st) {
  require("dwconv_wgrad", s, dtype, {x, dy, dw, ws});
  const WgradPlan p = wgrad_plan(s, dtype);
  DwWgradArgs a{};
  a.x = x, a.dy = dy, a.ws = ws;
  a.N = s.N, a.H = s.H, a.W = s.W, a.C = s.C, a.R = s.R, a.S = s.S;
  a.P = out_dim(s.H, s.ph, s.dh, s.R, s.sh), a.Q = out_dim(s.W, s.pw, s.dw, s.S, s.sw);
  a.sh = s.sh, a.sw = s.sw, a.ph = s.ph, a.pw = s.pw, a.dh = s.dh, a.dw = s.dw;
  a.TP = p.TP, a.lq = p.lq, a.PH = p.PH, a.PW = p.PW, a.NS = p.NS;
  a.tiles_p = p.tiles_p, a.tiles_q = p.tiles_q, a.cslices = p.cslices;
  a.ntiles = p.ntiles, a.tiles_per_chunk = p.tiles_per_chunk;
  const int64_t blocks = p.chunks * p.cslices;
  if (blocks >= (int64_t(1) << 31)) throw std::invalid_argument("dwconv_wgrad: grid too large");
  if (dtype == kBF16)
    hipLaunchKernelGGL(dw_wgrad_kernel<bf16>, dim3(static_cast<unsigned>(blocks)), dim3(NT), p.lds, st, a);
  else
    hipLaunchKernelGGL(dw_wgrad_kernel<float>, dim3(static_cast<unsigned>(blocks)), dim3(NT), p.lds, st, a);
  FFK_LAUNCH_CHECK("dwconv_wgrad");
  const int rsc = s.R * s.S * s.C;
  hipLaunchKernelGGL(dw_wgrad_reduce_kernel, dim3((rsc + NT - 1) / NT), dim3(NT), 0, st, ws, dw,
                     static_cast<int>(p.chunks), s.R * s.S, s.C);
  FFK_LAUNCH_CHECK("dwconv_wgrad");
}

}  // namespace ffk
