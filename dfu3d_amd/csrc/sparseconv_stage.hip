// sparseconv_stage.hip -- SURVEY.md §8 row f-20: sparse 3-D convolution (csrc/dfu3d_spc.h): the index plan of
// SubMConv3d / SparseConv3d, the forward sum and both gradients, every result a pure function of the inputs.
//
// The index plan is the machinery of hardvoxel_stage.hip once more.  A tensor's sites live in an open-addressing hash
// over 64-bit cell keys (compare-and-swap on the key, linear probing, load at most 1 / DFU3D_SPC_TABLE_PER_ROW) whose
// value is the row that owns the cell.  For the input tensor that is an integer atomicMin of the row; for the output of
// a strided layer it is the rank of the cell's first candidate (input row, offset) among all first candidates: an
// atomicMin of the candidate index, then an ordered scan of the flag "is the first candidate of its cell" (block
// counts, one workgroup scans them, every block ranks its own candidates).  Which entry a cell gets depends on the
// arrival order, nothing that is kept does.  No sort.
//
//   k_spc_fill      fills: table keys and one to three int blocks
//   k_spc_insert    a thread per input row: the cell's entry, atomicMin of the row, the status bits
//   k_spc_cand      a thread per candidate (row, K): the output cell's entry, atomicMin of the candidate
//   k_spc_count     a workgroup per 1024 candidates: first candidates of the block
//   k_spc_offsets   one workgroup: prefix over the blocks, the output count
//   k_spc_assign    a workgroup per 1024 candidates: a first candidate gives its cell the rank and writes out_indices
//   k_spc_tables    a thread per (output row, K): nbr, and inv where the neighbour exists
//
// The products are output-stationary.  k_spc_gemm<WN, TR>: a workgroup of four waves owns 32 * 4 / WN rows by 32 * WN
// channels; it keeps the tile's part of the table in LDS, leaves out the offsets no row of the tile has, stages the
// gathered rows and the weight slice of DFU3D_SPC_TILE_K channels in LDS and accumulates with the f32-input matrix
// instruction (32x32x2: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), k ascending -- THE SUM's chain, two steps at a time);
// every output element is written once.  TR reads the weight transposed and the inverse table: the feature gradient.
// k_spc_wgrad: a wave owns 32 x 32 weights of one offset and one chunk of rows; both operands of the matrix instruction
// are coalesced global loads (a row of dy, a gathered row of x), k runs over the rows.  k_spc_wsum adds the chunks in
// float64.  (The matrix instruction equals the fmaf chain bit for bit on gfx950: tests/test_gpu_sparse_conv.py.)
#include <limits.h>

#include "common.hpp"
#include "dfu3d_spc.h"

namespace {

constexpr int PT = DFU3D_SPC_ROW_THREADS;
constexpr int PW = PT / 64;
constexpr int GT = DFU3D_SPC_GEMM_THREADS;
constexpr int WT = DFU3D_SPC_WGRAD_THREADS;
constexpr int TK = DFU3D_SPC_TILE_K;
constexpr int MAXKV = DFU3D_SPC_MAX_KV;
constexpr int CHUNK = DFU3D_SPC_WGRAD_CHUNK;
constexpr unsigned long long EMPTY = ~0ull;
static_assert(PT == 1024 && GT == 256 && WT == 64 && TK == 32 && MAXKV <= 32 && CHUNK % 2 == 0, "the kernels' shapes");

typedef float f32x16 __attribute__((ext_vector_type(16)));

inline size_t up16(size_t v) { return (v + 15u) & ~(size_t)15u; }

// entries of the cell table of a tensor of n rows
inline long long sp_entries(long long n) {
  long long h = 16;
  while (h < (long long)DFU3D_SPC_TABLE_PER_ROW * n) h *= 2;
  return h;
}
inline size_t sp_table_bytes(long long n) { return (size_t)sp_entries(n) * 12u; }

struct SpTable {
  unsigned long long *keys;
  int *rows;
  unsigned mask;
};
inline SpTable sp_table(const void *p, long long n) {
  const long long h = sp_entries(n);
  return SpTable{(unsigned long long *)p, (int *)((char *)p + (size_t)h * 8u), (unsigned)(h - 1)};
}

struct SpGeom {
  int B, D, H, W;                                       // the input shape
  int kz, ky, kx, sz, sy, sx, pz, py, px;
  int oD, oH, oW;
  int KV;
};

// THE layout of the scratch of dfu3d_spc_downsample; the size is its last field
struct SpScratch {
  size_t cand_slot;                                     // int32 (N_in * KV): the candidate's entry of the output table or -1
  size_t first;                                         // int32 (entries of the output table): the first candidate
  size_t pre;                                           // int32 (blocks + 1): first candidates before a block
  size_t bytes;
  long long total, blocks;
};
SpScratch sp_scratch(long long N_in, long long N_out_cap, int KV) {
  SpScratch s;
  s.total = N_in * KV;
  s.blocks = s.total > 0 ? (s.total + PT - 1) / PT : 1;  // (no candidate: one block that counts nothing)
  size_t o = 0;
  s.cand_slot = o; o += up16((size_t)s.total * 4);
  s.first = o; o += up16((size_t)sp_entries(N_out_cap) * 4);
  s.pre = o; o += up16(((size_t)s.blocks + 1) * 4);
  s.bytes = o;
  return s;
}

__device__ __forceinline__ int sp_count(const int *__restrict__ count, int N) { return min(max(count[0], 0), N); }
__device__ __forceinline__ bool sp_cell_ok(int b, int z, int y, int x, int B, int D, int H, int W) {
  return (unsigned)b < (unsigned)B && (unsigned)z < (unsigned)D && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
}
__device__ __forceinline__ unsigned long long sp_key(int b, int z, int y, int x, int D, int H, int W) {
  return (((unsigned long long)b * D + z) * (unsigned long long)H + y) * (unsigned long long)W + x;
}
// the row that owns the cell, or -1
__device__ __forceinline__ int sp_lookup(const SpTable &T, unsigned long long key) {
  unsigned h = (unsigned)mix64(key) & T.mask;
  for (unsigned probe = 0; probe <= T.mask; probe++) {
    const unsigned long long cur = T.keys[h];
    if (cur == key) return T.rows[h];
    if (cur == EMPTY) return -1;
    h = (h + 1u) & T.mask;
  }
  return -1;
}
// the entry of the key, taking an empty one if it has none (the load is at most 1/2: an empty entry is always met)
__device__ __forceinline__ int sp_claim(const SpTable &T, unsigned long long key) {
  unsigned h = (unsigned)mix64(key) & T.mask;
  for (unsigned probe = 0; probe <= T.mask; probe++) {
    unsigned long long cur = __hip_atomic_load(&T.keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == EMPTY) cur = atomicCAS(&T.keys[h], EMPTY, key);
    if (cur == EMPTY || cur == key) return (int)h;
    h = (h + 1u) & T.mask;
  }
  return -1;
}

__global__ __launch_bounds__(PT) void k_spc_fill(unsigned long long *keys, long long nk, int *a, long long na, int va,
                                                 int *b, long long nb, int vb, int *c, long long nc, int vc) {
  const long long tid = (long long)blockIdx.x * PT + threadIdx.x, nth = (long long)gridDim.x * PT;
  for (long long i = tid; i < nk; i += nth) keys[i] = EMPTY;
  for (long long i = tid; i < na; i += nth) a[i] = va;
  for (long long i = tid; i < nb; i += nth) b[i] = vb;
  for (long long i = tid; i < nc; i += nth) c[i] = vc;
}

__global__ __launch_bounds__(PT) void k_spc_insert(const int *__restrict__ indices, const int *__restrict__ count, int N,
                                                   int B, int D, int H, int W, SpTable T, int *status) {
  const long long gl = (long long)blockIdx.x * PT + threadIdx.x;
  if (gl >= sp_count(count, N)) return;
  const int i = (int)gl;
  const int4 r = ((const int4 *)indices)[i];
  if (!sp_cell_ok(r.x, r.y, r.z, r.w, B, D, H, W)) {
    atomicOr(status, DFU3D_SPC_ST_BAD_COORD);
    return;
  }
  const int slot = sp_claim(T, sp_key(r.x, r.y, r.z, r.w, D, H, W));
  if (slot < 0) return;
  if (atomicMin(&T.rows[slot], i) != INT_MAX) atomicOr(status, DFU3D_SPC_ST_DUP_SITE);
}

// the output cell of input cell (z, y, x) through offset K, if whole and inside
__device__ __forceinline__ bool sp_out_cell(const SpGeom &G, int K, int z, int y, int x, int &oz, int &oy, int &ox) {
  const int jx = K % G.kx, jy = (K / G.kx) % G.ky, jz = K / (G.kx * G.ky);
  const int tz = z + G.pz - jz, ty = y + G.py - jy, tx = x + G.px - jx;
  if (tz < 0 || ty < 0 || tx < 0 || tz % G.sz || ty % G.sy || tx % G.sx) return false;
  oz = tz / G.sz;
  oy = ty / G.sy;
  ox = tx / G.sx;
  return oz < G.oD && oy < G.oH && ox < G.oW;
}

__global__ __launch_bounds__(PT) void k_spc_cand(const int *__restrict__ in_indices, const int *__restrict__ in_count,
                                                 int N_in, SpTable Tin, SpGeom G, SpTable Tout, int *first,
                                                 int *cand_slot, long long total) {
  const long long c = (long long)blockIdx.x * PT + threadIdx.x;
  if (c >= total) return;
  const int i = (int)(c / G.KV), K = (int)(c - (long long)i * G.KV);
  int slot = -1;
  if (i < sp_count(in_count, N_in)) {
    const int4 r = ((const int4 *)in_indices)[i];
    int oz, oy, ox;
    if (sp_cell_ok(r.x, r.y, r.z, r.w, G.B, G.D, G.H, G.W) && sp_out_cell(G, K, r.y, r.z, r.w, oz, oy, ox) &&
        sp_lookup(Tin, sp_key(r.x, r.y, r.z, r.w, G.D, G.H, G.W)) == i) {
      slot = sp_claim(Tout, sp_key(r.x, oz, oy, ox, G.oD, G.oH, G.oW));
      if (slot >= 0) atomicMin(&first[slot], (int)c);
    }
  }
  cand_slot[c] = slot;
}

__device__ __forceinline__ int sp_is_first(long long c, long long total, const int *__restrict__ cand_slot,
                                           const int *__restrict__ first, int &slot) {
  slot = c < total ? cand_slot[c] : -1;
  return (slot >= 0 && first[slot] == (int)c) ? 1 : 0;
}

__global__ __launch_bounds__(PT) void k_spc_count(long long total, const int *__restrict__ cand_slot,
                                                  const int *__restrict__ first, int *pre) {
  __shared__ int s_w[PW];
  int slot;
  const int flag = sp_is_first((long long)blockIdx.x * PT + threadIdx.x, total, cand_slot, first, slot);
  const int tot = block_sum_i<PW>(flag, s_w);
  if (threadIdx.x == 0) pre[blockIdx.x] = tot;
}

__global__ __launch_bounds__(PT) void k_spc_offsets(int blocks, int *pre, int *out_count) {
  __shared__ int s_w[PW];
  const int tot = block_scan_range<PT, 4, int, int>(blocks, [&](int i) { return pre[i]; },
                                                    [&](int i, int v) { pre[i] = v; }, s_w);
  if (threadIdx.x == 0) {
    pre[blocks] = tot;
    out_count[0] = tot;
  }
}

__global__ __launch_bounds__(PT) void k_spc_assign(const int *__restrict__ in_indices, SpGeom G, long long total,
                                                   const int *__restrict__ cand_slot, const int *__restrict__ first,
                                                   const int *__restrict__ pre, int N_out_cap, int *out_rows,
                                                   int *out_indices) {
  __shared__ int s_w[PW];
  const long long c = (long long)blockIdx.x * PT + threadIdx.x;
  int slot, tot;
  const int flag = sp_is_first(c, total, cand_slot, first, slot);
  const int ex = block_excl_scan<PW>(flag, s_w, tot);
  if (!flag) return;
  const int rank = pre[blockIdx.x] + ex;
  if (rank >= N_out_cap) return;                            // (cannot happen: THE CAPACITY BOUND)
  out_rows[slot] = rank;
  const int i = (int)(c / G.KV), K = (int)(c - (long long)i * G.KV);
  const int4 r = ((const int4 *)in_indices)[i];
  int oz = 0, oy = 0, ox = 0;
  sp_out_cell(G, K, r.y, r.z, r.w, oz, oy, ox);
  ((int4 *)out_indices)[rank] = make_int4(r.x, oz, oy, ox);
}

__global__ __launch_bounds__(PT) void k_spc_tables(int N_in, SpTable Tin, const int *__restrict__ out_indices,
                                                   const int *__restrict__ out_count, int N_out, SpTable Tout, SpGeom G,
                                                   int *nbr, int *inv) {
  const long long t = (long long)blockIdx.x * PT + threadIdx.x;
  if (t >= (long long)N_out * G.KV) return;
  const int o = (int)(t / G.KV), K = (int)(t - (long long)o * G.KV);
  int r = -1;
  if (o < sp_count(out_count, N_out)) {
    const int4 c = ((const int4 *)out_indices)[o];
    if (sp_cell_ok(c.x, c.y, c.z, c.w, G.B, G.oD, G.oH, G.oW) &&
        sp_lookup(Tout, sp_key(c.x, c.y, c.z, c.w, G.oD, G.oH, G.oW)) == o) {
      const int jx = K % G.kx, jy = (K / G.kx) % G.ky, jz = K / (G.kx * G.ky);
      const int iz = c.y * G.sz - G.pz + jz, iy = c.z * G.sy - G.py + jy, ix = c.w * G.sx - G.px + jx;
      if (sp_cell_ok(c.x, iz, iy, ix, G.B, G.D, G.H, G.W)) r = sp_lookup(Tin, sp_key(c.x, iz, iy, ix, G.D, G.H, G.W));
      if ((unsigned)r >= (unsigned)N_in) r = -1;
    }
  }
  nbr[t] = r;
  if (r >= 0) inv[(long long)r * G.KV + K] = o;
}

// row of the 32 x 32 result that register r of a lane in half h holds (the column is lane & 31)
__device__ __forceinline__ int mfma_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// out[r][n] = sum over K, m of src[tab[r][K]][m] * W(n, K, m); W(n, K, m) = w[(n * KV + K) * Cm + m] (TR false: forward,
// m = ci, n = co) or w[(m * KV + K) * Cn + n] (TR true: feature gradient, m = co, n = ci)
template <int WN, bool TR>
__global__ __launch_bounds__(GT) void k_spc_gemm(const float *__restrict__ src, int n_src, const int *__restrict__ tab,
                                                 int n_rows, int KV, const float *__restrict__ w, int Cm, int Cn,
                                                 float *__restrict__ out) {
  constexpr int TM = 32 * (4 / WN), TN = 32 * WN;
  constexpr int WS = TR ? TK * (TN + 1) : TN * (TK + 1);
  __shared__ int s_tab[TM * MAXKV];
  __shared__ float xs[TM * (TK + 1)];
  __shared__ float ws[WS];
  __shared__ unsigned s_mask;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
  const int row0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
  const int wr0 = (wave / WN) * 32, wn0 = (wave % WN) * 32;
  if (t == 0) s_mask = 0u;
  __syncthreads();
  unsigned mine = 0u;
  for (int idx = t; idx < TM * KV; idx += GT) {
    const int r = idx / KV, K = idx - r * KV;
    int v = -1;
    if (row0 + r < n_rows) {
      v = tab[(size_t)(row0 + r) * KV + K];
      if ((unsigned)v >= (unsigned)n_src) v = -1;
    }
    s_tab[idx] = v;
    if (v >= 0) mine |= 1u << K;
  }
  if (mine) atomicOr(&s_mask, mine);
  __syncthreads();
  const unsigned present = s_mask;
  const bool wave_has_cols = n0 + wn0 < Cn;                 // (uniform in the wave)
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.0f;
  for (int K = 0; K < KV; K++) {
    if (!((present >> K) & 1u)) continue;                   // (uniform) no row of the tile has this neighbour
    for (int c0 = 0; c0 < Cm; c0 += TK) {
      for (int idx = t; idx < TM * TK; idx += GT) {
        const int r = idx >> 5, c = idx & 31;
        const int row = s_tab[r * KV + K];
        float v = 0.0f;
        if (row >= 0 && c0 + c < Cm) v = src[(size_t)row * Cm + c0 + c];
        xs[r * (TK + 1) + c] = v;
      }
      if (!TR) {
        for (int idx = t; idx < TN * TK; idx += GT) {
          const int n = idx >> 5, c = idx & 31;
          float v = 0.0f;
          if (n0 + n < Cn && c0 + c < Cm) v = w[((size_t)(n0 + n) * KV + K) * Cm + c0 + c];
          ws[n * (TK + 1) + c] = v;
        }
      } else {
        for (int idx = t; idx < TK * TN; idx += GT) {
          const int c = idx / TN, n = idx - c * TN;
          float v = 0.0f;
          if (n0 + n < Cn && c0 + c < Cm) v = w[((size_t)(c0 + c) * KV + K) * Cn + n0 + n];
          ws[c * (TN + 1) + n] = v;
        }
      }
      __syncthreads();
      const int klen = min(TK, Cm - c0);
      if (wave_has_cols) {
        for (int s = 0; s < (klen + 1) / 2; s++) {          // (uniform; column klen of an odd klen holds +0.0)
          const int kk = 2 * s + half;
          const float a = xs[(wr0 + l31) * (TK + 1) + kk];
          const float b = TR ? ws[kk * (TN + 1) + wn0 + l31] : ws[(wn0 + l31) * (TK + 1) + kk];
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }
  if (!wave_has_cols) return;
  const int col = n0 + wn0 + l31;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int orow = row0 + wr0 + mfma_row(r, half);
    if (orow < n_rows && col < Cn) out[(size_t)orow * Cn + col] = acc[r];
  }
}

// one chunk's partial of 32 x 32 weights of offset K: part[chunk][co][K][ci]
__global__ __launch_bounds__(WT) void k_spc_wgrad(const float *__restrict__ x, int N_in, const float *__restrict__ dy,
                                                  const int *__restrict__ nbr, int N_out, int KV, int Cin, int Cout,
                                                  int tiles_ci, int tiles, float *__restrict__ part) {
  const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
  const int chunk = blockIdx.x / tiles, tile = blockIdx.x - chunk * tiles, K = blockIdx.y;
  const int co0 = (tile / tiles_ci) * 32, ci0 = (tile % tiles_ci) * 32;
  const int o0 = chunk * CHUNK, o1 = min(o0 + CHUNK, N_out);
  const int co = co0 + l31, ci = ci0 + l31;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.0f;
  for (int o = o0; o < o1; o += 2) {
    const int oo = o + half;
    float a = 0.0f, b = 0.0f;
    if (oo < o1) {
      if (co < Cout) a = dy[(size_t)oo * Cout + co];
      const int r = nbr[(size_t)oo * KV + K];
      if ((unsigned)r < (unsigned)N_in && ci < Cin) b = x[(size_t)r * Cin + ci];
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  }
  if (ci >= Cin) return;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int c = co0 + mfma_row(r, half);
    if (c < Cout) part[(((size_t)chunk * Cout + c) * KV + K) * Cin + ci] = acc[r];
  }
}

__global__ __launch_bounds__(256) void k_spc_wsum(const float *__restrict__ part, int chunks, int elems,
                                                  float *__restrict__ dw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= elems) return;
  double s = 0.0;
  for (int c = 0; c < chunks; c++) s += (double)part[(size_t)c * elems + e];
  dw[e] = (float)s;
}

// ---- the host side ---------------------------------------------------------------------------------------------------
int sp_sizes(int B, const int32_t *shape) {
  if (B < 1 || shape[0] < 1 || shape[1] < 1 || shape[2] < 1) return DFU3D_EINVAL;
  if (B > DFU3D_SPC_MAX_BATCH) return DFU3D_ERANGE;
  unsigned __int128 cells = (unsigned __int128)B;
  for (int j = 0; j < 3; j++) cells *= (unsigned __int128)shape[j];
  return cells >= ((unsigned __int128)1 << DFU3D_SPC_KEY_BITS) ? DFU3D_ERANGE : DFU3D_OK;
}

// the geometry of a layer; DFU3D_EINVAL for what no layer has
int sp_geom(int B, const int32_t *shape, const int32_t *k, const int32_t *s, const int32_t *p, SpGeom &G) {
  int out[3];
  for (int j = 0; j < 3; j++) {
    if ((k[j] != 1 && k[j] != 3) || (s[j] != 1 && s[j] != 2) || p[j] < 0 || p[j] >= k[j]) return DFU3D_EINVAL;
    const long long num = (long long)shape[j] + 2 * p[j] - k[j];
    if (num < 0) return DFU3D_EINVAL;
    out[j] = (int)(num / s[j]) + 1;
  }
  G = SpGeom{B, shape[0], shape[1], shape[2], k[0], k[1], k[2], s[0], s[1], s[2], p[0], p[1], p[2],
             out[0], out[1], out[2], k[0] * k[1] * k[2]};
  return DFU3D_OK;
}

// THE CAPACITY BOUND
long long sp_bound(const SpGeom &G, long long N_in) {
  const long long reach = (long long)((G.kz + G.sz - 1) / G.sz) * ((G.ky + G.sy - 1) / G.sy) * ((G.kx + G.sx - 1) / G.sx);
  const unsigned __int128 cells = (unsigned __int128)G.B * G.oD * G.oH * G.oW;
  const long long by_rows = N_in * reach;
  return cells < (unsigned __int128)by_rows ? (long long)cells : by_rows;
}

unsigned sp_grid(long long n, int per) {
  const long long b = (n + per - 1) / per;
  return (unsigned)(b > 0 ? b : 1);
}
unsigned sp_fill_grid(long long n) {
  const long long b = (n + PT - 1) / PT;
  return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

int sp_gemm_args(const void *src, int n_src, const void *tab, int n_rows, int KV, const void *w, int Cin, int Cout,
                 const void *out) {
  if (n_src < 0 || n_rows < 0 || KV < 1 || KV > DFU3D_SPC_MAX_KV || Cin < 1 || Cout < 1) return DFU3D_EINVAL;
  if (!w || (n_src > 0 && !src) || (n_rows > 0 && (!tab || !out))) return DFU3D_EINVAL;
  if (Cin > DFU3D_SPC_MAX_CHANNELS || Cout > DFU3D_SPC_MAX_CHANNELS || n_src > DFU3D_SPC_MAX_ROWS ||
      n_rows > DFU3D_SPC_MAX_ROWS)
    return DFU3D_ERANGE;
  return DFU3D_OK;
}

template <bool TR>
int sp_gemm(const float *src, int n_src, const int *tab, int n_rows, int KV, const float *w, int Cm, int Cn, float *out,
            hipStream_t st) {
  if (Cn <= 32) {
    hipLaunchKernelGGL((k_spc_gemm<1, TR>), dim3(sp_grid(n_rows, 128), 1), dim3(GT), 0, st, src, n_src, tab, n_rows, KV, w,
                       Cm, Cn, out);
  } else {
    hipLaunchKernelGGL((k_spc_gemm<2, TR>), dim3(sp_grid(n_rows, 64), (unsigned)((Cn + 63) / 64)), dim3(GT), 0, st, src,
                       n_src, tab, n_rows, KV, w, Cm, Cn, out);
  }
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

}  // namespace

static_assert(DFU3D_SPC_LAUNCHES_INDEX == 2, "fill, insert");
static_assert(DFU3D_SPC_LAUNCHES_DOWNSAMPLE == 5, "fill, cand, count, offsets, assign");
static_assert(DFU3D_SPC_LAUNCHES_TABLES == 2, "fill, tables");
static_assert(DFU3D_SPC_LAUNCHES_WGRAD == 2, "wgrad, wsum");

extern "C" int32_t dfu3d_spc_version(void) { return DFU3D_SPC_VERSION; }

extern "C" size_t dfu3d_spc_table_bytes(int32_t N_cap) {
  if (N_cap < 0 || N_cap > DFU3D_SPC_MAX_ROWS) return 0;
  return sp_table_bytes(N_cap);
}

extern "C" size_t dfu3d_spc_scratch_bytes(int32_t N_in, int32_t N_out_cap, int32_t KV) {
  if (N_in < 0 || N_out_cap < 1 || KV < 1 || KV > DFU3D_SPC_MAX_KV || N_in > DFU3D_SPC_MAX_ROWS ||
      N_out_cap > DFU3D_SPC_MAX_ROWS || (long long)N_in * KV > (long long)INT_MAX)
    return 0;
  return sp_scratch(N_in, N_out_cap, KV).bytes;
}

extern "C" size_t dfu3d_spc_wgrad_scratch_bytes(int32_t N_out, int32_t KV, int32_t Cin, int32_t Cout) {
  if (N_out < 0 || N_out > DFU3D_SPC_MAX_ROWS || KV < 1 || KV > DFU3D_SPC_MAX_KV || Cin < 1 || Cout < 1 ||
      Cin > DFU3D_SPC_MAX_CHANNELS || Cout > DFU3D_SPC_MAX_CHANNELS)
    return 0;
  const size_t chunks = ((size_t)N_out + CHUNK - 1) / CHUNK;
  return up16(chunks * (size_t)Cout * KV * Cin * 4u);
}

extern "C" int dfu3d_spc_index(const int32_t *indices, const int32_t *count, int32_t N, int32_t B, const int32_t *shape,
                               void *table, size_t table_bytes, int32_t *status, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!count || !shape || !table || !status || N < 0 || (N > 0 && !indices)) return DFU3D_EINVAL;
  const int rc = sp_sizes(B, shape);
  if (rc != DFU3D_OK) return rc;
  if (N > DFU3D_SPC_MAX_ROWS) return DFU3D_ERANGE;
  if (((uintptr_t)table & 15u) || table_bytes < sp_table_bytes(N)) return DFU3D_EINVAL;
  if (N > 0 && ((uintptr_t)indices & 15u)) return DFU3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const SpTable T = sp_table(table, N);
  const long long Hn = (long long)T.mask + 1;
  hipLaunchKernelGGL(k_spc_fill, dim3(sp_fill_grid(Hn)), dim3(PT), 0, st, T.keys, Hn, T.rows, Hn, INT_MAX, (int *)nullptr,
                     0ll, 0, (int *)nullptr, 0ll, 0);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_spc_insert, dim3(sp_grid(N, PT)), dim3(PT), 0, st, (const int *)indices, (const int *)count, N, B,
                     shape[0], shape[1], shape[2], T, (int *)status);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_spc_downsample(const int32_t *in_indices, const int32_t *in_count, int32_t N_in, const void *in_table,
                                    int32_t B, const int32_t *in_shape, const int32_t *ksize, const int32_t *stride,
                                    const int32_t *padding, int32_t N_out_cap, void *scratch, size_t scratch_bytes,
                                    int32_t *out_indices, int32_t *out_count, void *out_table, size_t out_table_bytes,
                                    void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!in_count || !in_table || !in_shape || !ksize || !stride || !padding || !scratch || !out_indices || !out_count ||
      !out_table || N_in < 0 || N_out_cap < 1 || (N_in > 0 && !in_indices))
    return DFU3D_EINVAL;
  int rc = sp_sizes(B, in_shape);
  if (rc != DFU3D_OK) return rc;
  SpGeom G;
  rc = sp_geom(B, in_shape, ksize, stride, padding, G);
  if (rc != DFU3D_OK) return rc;
  if (N_in > DFU3D_SPC_MAX_ROWS || N_out_cap > DFU3D_SPC_MAX_ROWS || (long long)N_in * G.KV > (long long)INT_MAX)
    return DFU3D_ERANGE;
  if ((long long)N_out_cap < sp_bound(G, N_in)) return DFU3D_EINVAL;
  const SpScratch S = sp_scratch(N_in, N_out_cap, G.KV);
  if (((uintptr_t)scratch & 15u) || scratch_bytes < S.bytes) return DFU3D_EINVAL;
  if (((uintptr_t)out_table & 15u) || out_table_bytes < sp_table_bytes(N_out_cap)) return DFU3D_EINVAL;
  if (((uintptr_t)out_indices & 15u) || (N_in > 0 && ((uintptr_t)in_indices & 15u)) || ((uintptr_t)in_table & 15u))
    return DFU3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  char *base = (char *)scratch;
  int *cand_slot = (int *)(base + S.cand_slot), *first = (int *)(base + S.first), *pre = (int *)(base + S.pre);
  const SpTable Tin = sp_table(in_table, N_in), Tout = sp_table(out_table, N_out_cap);
  const long long Hn = (long long)Tout.mask + 1;
  hipLaunchKernelGGL(k_spc_fill, dim3(sp_fill_grid(Hn > 4ll * N_out_cap ? Hn : 4ll * N_out_cap)), dim3(PT), 0, st, Tout.keys,
                     Hn, Tout.rows, Hn, -1, first, Hn, INT_MAX, (int *)out_indices, 4ll * N_out_cap, -1);
  DFU3D_LAUNCH_CHECK();
  const unsigned cgrid = sp_grid(S.total, PT);
  hipLaunchKernelGGL(k_spc_cand, dim3(cgrid), dim3(PT), 0, st, (const int *)in_indices, (const int *)in_count, N_in, Tin, G,
                     Tout, first, cand_slot, S.total);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_spc_count, dim3(cgrid), dim3(PT), 0, st, S.total, (const int *)cand_slot, (const int *)first, pre);
  DFU3D_LAUNCH_CHECK();
  // (with no candidate at all the one block of the count kernel writes pre[0] = 0 and the scan runs over it)
  hipLaunchKernelGGL(k_spc_offsets, dim3(1), dim3(PT), 0, st, (int)cgrid, pre, (int *)out_count);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_spc_assign, dim3(cgrid), dim3(PT), 0, st, (const int *)in_indices, G, S.total,
                     (const int *)cand_slot, (const int *)first, (const int *)pre, N_out_cap, Tout.rows,
                     (int *)out_indices);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_spc_tables(int32_t N_in, const void *in_table, int32_t in_table_rows, const int32_t *out_indices,
                                const int32_t *out_count, int32_t N_out, const void *out_table, int32_t out_table_rows,
                                int32_t B, const int32_t *in_shape, const int32_t *ksize, const int32_t *stride,
                                const int32_t *padding, int32_t *nbr, int32_t *inv, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  if (!in_table || !out_table || !out_count || !in_shape || !ksize || !stride || !padding || N_in < 0 || N_out < 0 ||
      in_table_rows < N_in || out_table_rows < N_out || (N_out > 0 && (!out_indices || !nbr)) || (N_in > 0 && !inv))
    return DFU3D_EINVAL;
  int rc = sp_sizes(B, in_shape);
  if (rc != DFU3D_OK) return rc;
  SpGeom G;
  rc = sp_geom(B, in_shape, ksize, stride, padding, G);
  if (rc != DFU3D_OK) return rc;
  if (in_table_rows > DFU3D_SPC_MAX_ROWS || out_table_rows > DFU3D_SPC_MAX_ROWS) return DFU3D_ERANGE;
  if (((uintptr_t)in_table & 15u) || ((uintptr_t)out_table & 15u) || (N_out > 0 && ((uintptr_t)out_indices & 15u)))
    return DFU3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const SpTable Tin = sp_table(in_table, in_table_rows), Tout = sp_table(out_table, out_table_rows);
  const long long ninv = (long long)N_in * G.KV;
  hipLaunchKernelGGL(k_spc_fill, dim3(sp_fill_grid(ninv)), dim3(PT), 0, st, (unsigned long long *)nullptr, 0ll, (int *)inv,
                     ninv, -1, (int *)nullptr, 0ll, 0, (int *)nullptr, 0ll, 0);
  DFU3D_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_spc_tables, dim3(sp_grid((long long)N_out * G.KV, PT)), dim3(PT), 0, st, N_in, Tin,
                     (const int *)out_indices, (const int *)out_count, N_out, Tout, G, (int *)nbr, (int *)inv);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}

extern "C" int dfu3d_spc_forward(const float *x, int32_t N_in, const int32_t *nbr, int32_t N_out, int32_t KV,
                                 const float *w, int32_t Cin, int32_t Cout, float *y, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  const int rc = sp_gemm_args(x, N_in, nbr, N_out, KV, w, Cin, Cout, y);
  if (rc != DFU3D_OK) return rc;
  if (N_out == 0) return DFU3D_OK;
  return sp_gemm<false>(x, N_in, (const int *)nbr, N_out, KV, w, Cin, Cout, y, (hipStream_t)stream);
}

extern "C" int dfu3d_spc_dgrad(const float *dy, int32_t N_out, const int32_t *inv, int32_t N_in, int32_t KV,
                               const float *w, int32_t Cin, int32_t Cout, float *dx, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  const int rc = sp_gemm_args(dy, N_out, inv, N_in, KV, w, Cin, Cout, dx);
  if (rc != DFU3D_OK) return rc;
  if (N_in == 0) return DFU3D_OK;
  return sp_gemm<true>(dy, N_out, (const int *)inv, N_in, KV, w, Cout, Cin, dx, (hipStream_t)stream);
}

extern "C" int dfu3d_spc_wgrad(const float *x, int32_t N_in, const float *dy, const int32_t *nbr, int32_t N_out, int32_t KV,
                               int32_t Cin, int32_t Cout, void *scratch, size_t scratch_bytes, float *dw, void *stream) {
  DFU3D_CLEAR_STALE_ERROR();
  const int rc = sp_gemm_args(x, N_in, nbr, N_out, KV, dw, Cin, Cout, dy);
  if (rc != DFU3D_OK) return rc;
  const size_t need = dfu3d_spc_wgrad_scratch_bytes(N_out, KV, Cin, Cout);
  if (need > 0 && (!scratch || ((uintptr_t)scratch & 15u) || scratch_bytes < need)) return DFU3D_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = (N_out + CHUNK - 1) / CHUNK;
  const int tiles_ci = (Cin + 31) / 32, tiles = tiles_ci * ((Cout + 31) / 32);
  const int elems = Cout * KV * Cin;
  if (chunks > 0) {
    hipLaunchKernelGGL(k_spc_wgrad, dim3((unsigned)(chunks * tiles), (unsigned)KV), dim3(WT), 0, st, x, N_in, dy,
                       (const int *)nbr, N_out, KV, Cin, Cout, tiles_ci, tiles, (float *)scratch);
    DFU3D_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_spc_wsum, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, (const float *)scratch, chunks,
                     elems, dw);
  DFU3D_LAUNCH_CHECK();
  return DFU3D_OK;
}
