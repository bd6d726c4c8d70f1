// Per-step graph build: torch_cluster.radius_graph (CUDA-kernel semantics) + union with the static
// bond/2-hop/3-hop edges + coalesce order, restated for one workgroup per molecule.
// Replaces models/common.py:208-233 (_extend_to_radius_graph) and geometry.py:5-6 (get_distance).
//
// Output (agdiff_ws_t): a destination-sorted CSR (edges of target i contiguous, sources ascending)
// plus `ref2dst`, the permutation from the reference's (src, dst)-sorted order.  Three launches:
//   count (per graph) -> scan over graphs (one workgroup) -> fill (per graph, lists recomputed).
#include "common.hpp"

namespace {

struct GraphArgs {
  const int32_t* graph_ptr;
  const int32_t* loc_in_ptr;
  const int32_t* loc_in_eid;
  const int32_t* loc_src;
  const int32_t* loc_type;
  const int32_t* loc_row;
  const float* pos;
  float r2;
  int32_t words;  // ceil(max_atoms_per_graph / 32)
  // outputs
  int32_t* graph_edge_cnt;
  const int32_t* graph_edge_ptr;
  int32_t* in_ptr;
  int32_t* out_ptr;
  int32_t* e_src;
  int32_t* e_dst;
  int32_t* e_type;
  float* e_len;
  int32_t* ref2dst;
  int32_t* e_loc;
  // canonical edges (one per undirected pair whose two directions carry the same type, plus every unpaired edge)
  int32_t* graph_canon_cnt;
  const int32_t* graph_canon_ptr;
  float* c_len;
  int32_t* c_type;
  int32_t* c_src;
  int32_t* c_dst;
  int32_t* c_pos;
  int32_t* c_mir;
  // radius edges (type 0) by target, AGDIFF_RAD_STRIDE rows per target (optional: rad_cnt may be null)
  int32_t* rad_cnt;
  int32_t* rad_src;
  float* rad_len;
  // canon_radius_only != 0: the canonical list holds radius edges only (the denoising loop: nothing but the global head
  // walks it then)
  int32_t canon_radius_only;
  // hand-over from the count pass to the fill pass (optional): the in-adjacency masks and the two degree arrays of every
  // molecule, so that the fill pass does not repeat the distance tests and the mirror look-ups
  uint32_t* g_inbits;    // [N][words]
  int32_t* g_deg;        // [N] in-degrees
  int32_t* g_cdeg;       // [N] canonical in-degrees
  int32_t num_graphs;
  // optional (r_scale != null): lw(d) * C(d) of the 2 * num_convs CFConvs for the radius rows, and the pad rows that complete
  // every target's last 16-row tile, straight from the fill pass (what agdiff_edge_scales_split(which = 0) does as a launch
  // of its own: 36 us alone, 70 us beside the local branch's kernels)
  const float* dw[2 * AGDIFF_MAX_CONVS];
  float* r_scale;
  int64_t rpad;
  int32_t n_scales;
  float cutoff;
  int32_t smooth;
};

// Edge lengths must come out bit-identical wherever they are computed (the per-step graph build and the local-edge
// pass feed the same encoder): hipcc lowers sqrtf differently from kernel to kernel (1 ulp apart), so the root is
// taken in double and rounded once -- correctly rounded for every float input.
__device__ __forceinline__ float ag_sqrt_rn(float x) { return (float)sqrt((double)x); }

// d^2 exactly as the restated rule: ((dx*dx + dy*dy) + dz*dz), no FMA contraction.
__device__ __forceinline__ float dist2_nofma(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return (xx + yy) + zz;
}

extern __shared__ uint32_t ag_graph_smem[];

// One workgroup per molecule, one WAVE per target atom at a time: the 64 lanes test 64 candidate sources at once,
// wave ballots replace the serial scan of the reference rule --
//   radius_graph: source j is kept for target i if d2(i, j) < r^2 and fewer than 33 such candidates (self
//   included) precede it in ascending j; self is then dropped; bond / 2-hop / 3-hop edges are always present
// -- and the position of an edge inside the target's list is the population count of the kept mask below its
// lane, so all per-edge stores are contiguous.  The in-adjacency masks stay in LDS (row i, bit j <=> edge j -> i);
// out-degrees and the (src, dst)-order permutation ref2dst come from their columns.
#define AG_GRAPH_THREADS 1024     // launch bound; the launcher picks 512 or 1024 threads per molecule
template <bool FILL>
__global__ void __launch_bounds__(AG_GRAPH_THREADS) k_graph(GraphArgs a) {
  const int g = blockIdx.x;
  const int g0 = a.graph_ptr[g];
  const int n = a.graph_ptr[g + 1] - g0;
  const int words = a.words;          // 32-bit words per mask row, even (whole 64-lane chunks)
  const int nmax = words * 32;
  // LDS carve: pos[3 nmax] | indeg[nmax] | outdeg[nmax] | canonical indeg[nmax] | inbits[nmax][words] | locbits[nmax][words]
  float* spos = reinterpret_cast<float*>(ag_graph_smem);
  int* sin = reinterpret_cast<int*>(ag_graph_smem + 3 * nmax);
  int* sout = sin + nmax;
  int* scan_c = sout + nmax;
  uint32_t* inbits = reinterpret_cast<uint32_t*>(scan_c + nmax);
  uint32_t* locbits = inbits + nmax * words;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));     // lanes below mine
  auto bit = [&](const uint32_t* rows, int r, int c) -> bool { return (rows[r * words + (c >> 5)] >> (c & 31)) & 1u; };
  auto rank_below = [&](const uint32_t* rows, int r, int c) -> int {   // set bits of row r below column c
    const uint32_t* row = rows + r * words;
    int k = __popc(row[c >> 5] & ((1u << (c & 31)) - 1u));
    for (int w = 0; w < (c >> 5); ++w) k += __popc(row[w]);
    return k;
  };
  auto local_type = [&](int i, int j) -> int {      // type of the local edge j -> i (caller checked its locbits bit)
    return a.loc_type[a.loc_in_eid[a.loc_in_ptr[g0 + i] + rank_below(locbits, i, j)]];
  };
  // The directed edges j -> i and i -> j are mirrors when both exist with the same type: same length, same type,
  // hence bit-identical edge_attr, filter and pair-head output (dualenc.py:189-211).  Canonical = the one with
  // src < dst, or any edge without a mirror.
  auto has_mirror = [&](int i, int j) -> bool {     // for an existing edge j -> i
    if (!bit(inbits, j, i)) return false;
    const bool li = bit(locbits, i, j), lj = bit(locbits, j, i);
    if (li != lj) return false;
    return !li || local_type(i, j) == local_type(j, i);
  };

  __shared__ float sseg[FILL ? 2 * AGDIFF_MAX_CONVS * 100 : 1];         // the CFConvs' distance-weighting segment tables
  if (FILL && a.r_scale)
    for (int i = threadIdx.x; i < a.n_scales * 100; i += blockDim.x) sseg[i] = a.dw[i / 100][i % 100];
  for (int i = threadIdx.x; i < 3 * n; i += blockDim.x) spos[i] = a.pos[3 * (size_t)g0 + i];
  // static local in-adjacency of the molecule: the thread that owns target i sets its row
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    for (int w = 0; w < words; ++w) locbits[i * words + w] = 0u;
    for (int k = a.loc_in_ptr[g0 + i]; k < a.loc_in_ptr[g0 + i + 1]; ++k) {
      const int j = a.loc_src[a.loc_in_eid[k]] - g0;
      locbits[i * words + (j >> 5)] |= 1u << (j & 31);
    }
  }
  __syncthreads();

  int wave_total = 0, wave_ctotal = 0;
  if (FILL && a.g_inbits) {
    // the count pass of this build left the masks and degrees in global memory
    for (int k = threadIdx.x; k < n * words; k += blockDim.x) inbits[k] = a.g_inbits[(size_t)g0 * words + k];
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      sin[i] = a.g_deg[g0 + i];
      scan_c[i] = a.g_cdeg[g0 + i];
    }
    __syncthreads();
  } else {
  // pass 1: kept masks and in-degrees
  for (int i = wave; i < n; i += nwaves) {
    const float xi = spos[3 * i], yi = spos[3 * i + 1], zi = spos[3 * i + 2];
    int cnt_r = 0, deg = 0;
    for (int c = 0; 64 * c < n; ++c) {
      const int j = 64 * c + lane;
      const bool valid = j < n;
      const int jj = valid ? j : 0;
      const float d2 = dist2_nofma(xi, yi, zi, spos[3 * jj], spos[3 * jj + 1], spos[3 * jj + 2]);
      const bool within = valid && d2 < a.r2;
      const uint64_t wmask = __ballot(within);
      const bool rad = within && (cnt_r + __popcll(wmask & lt) < AGDIFF_RADIUS_CAP) && j != i;
      cnt_r += __popcll(wmask);
      const bool loc = valid && ((locbits[i * words + 2 * c + (lane >> 5)] >> (lane & 31)) & 1u);
      const uint64_t emask = __ballot(rad || loc);
      if (lane == 0) {
        inbits[i * words + 2 * c] = (uint32_t)emask;
        inbits[i * words + 2 * c + 1] = (uint32_t)(emask >> 32);
      }
      deg += __popcll(emask);
    }
    if (lane == 0) sin[i] = deg;
    wave_total += deg;
  }
  __syncthreads();

  // canonical in-degrees (needs every row of inbits: after the barrier)
  for (int i = wave; i < n; i += nwaves) {
    int cdeg = 0;
    for (int c = 0; 64 * c < n; ++c) {
      const int j = 64 * c + lane;
      const bool e = j < n && bit(inbits, i, j);
      bool canon;
      if (a.canon_radius_only) {       // radius edges: a mirror is the radius edge the other way round (same length)
        const bool rad = e && !bit(locbits, i, j);
        canon = rad && (j < i || !(bit(inbits, j, i) && !bit(locbits, j, i)));
      } else {
        canon = e && (j < i || !has_mirror(i, j));
      }
      cdeg += __popcll(__ballot(canon));
    }
    if (lane == 0) scan_c[i] = cdeg;
    wave_ctotal += cdeg;
  }
  __syncthreads();
  if (!FILL && a.g_inbits) {        // hand the masks and degrees over to the fill pass
    for (int k = threadIdx.x; k < n * words; k += blockDim.x) a.g_inbits[(size_t)g0 * words + k] = inbits[k];
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      a.g_deg[g0 + i] = sin[i];
      a.g_cdeg[g0 + i] = scan_c[i];
    }
  }
  }

  if (!FILL) {
    __shared__ int wsum[2][AG_GRAPH_THREADS / 64];
    if (lane == 0) { wsum[0][wave] = wave_total; wsum[1][wave] = wave_ctotal; }
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0, ctot = 0;
      for (int w = 0; w < nwaves; ++w) { tot += wsum[0][w]; ctot += wsum[1][w]; }
      a.graph_edge_cnt[g] = tot;
      a.graph_canon_cnt[g] = ctot;
    }
    return;
  }

  // out-degrees = column counts of the in-adjacency
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    int c = 0;
    for (int i = 0; i < n; ++i) c += (inbits[i * words + (j >> 5)] >> (j & 31)) & 1u;
    sout[j] = c;
  }
  __syncthreads();
  // inclusive scans of sin / sout / scan_c (n <= 512): Hillis-Steele in place, three arrays together
  for (int off = 1; off < n; off <<= 1) {
    int vi[2], vo[2], vc[2], cnt = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x, ++cnt) {
      vi[cnt] = sin[i] + (i >= off ? sin[i - off] : 0);
      vo[cnt] = sout[i] + (i >= off ? sout[i - off] : 0);
      vc[cnt] = scan_c[i] + (i >= off ? scan_c[i - off] : 0);
    }
    __syncthreads();
    cnt = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x, ++cnt) {
      sin[i] = vi[cnt];
      sout[i] = vo[cnt];
      scan_c[i] = vc[cnt];
    }
    __syncthreads();
  }
  const int base = a.graph_edge_ptr[g];
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    a.in_ptr[g0 + i] = base + (i ? sin[i - 1] : 0);
    a.out_ptr[g0 + i] = base + (i ? sout[i - 1] : 0);
  }
  if (g == a.num_graphs - 1 && threadIdx.x == 0) {
    a.in_ptr[g0 + n] = base + (n ? sin[n - 1] : 0);
    a.out_ptr[g0 + n] = base + (n ? sout[n - 1] : 0);
  }
  // pass 2: emit the lists, one wave per target, contiguous stores
  for (int i = wave; i < n; i += nwaves) {
    const float xi = spos[3 * i], yi = spos[3 * i + 1], zi = spos[3 * i + 2];
    int p0 = base + (i ? sin[i - 1] : 0);
    int cp0 = a.graph_canon_ptr[g] + (i ? scan_c[i - 1] : 0);
    int lk = a.loc_in_ptr[g0 + i];
    int rp0 = (g0 + i) * AGDIFF_RAD_STRIDE;        // the target's own rows of the radius list (at most AGDIFF_RADIUS_CAP used)
    for (int c = 0; 64 * c < n; ++c) {
      const int j = 64 * c + lane;
      const int jj = (j < n) ? j : 0;
      const uint64_t emask = (uint64_t)inbits[i * words + 2 * c] | ((uint64_t)inbits[i * words + 2 * c + 1] << 32);
      const uint64_t lmask = (uint64_t)locbits[i * words + 2 * c] | ((uint64_t)locbits[i * words + 2 * c + 1] << 32);
      const uint64_t rmask = emask & ~lmask;
      const bool e = (emask >> lane) & 1ull;
      bool mir, canon;
      if (a.canon_radius_only) {
        const bool rad = (rmask >> lane) & 1ull;
        mir = rad && bit(inbits, j, i) && !bit(locbits, j, i);
        canon = rad && (j < i || !mir);
      } else {
        mir = e && has_mirror(i, j);
        canon = e && (j < i || !mir);
      }
      const uint64_t cmask = __ballot(canon);
      if (e) {
        const int p = p0 + __popcll(emask & lt);
        int ty = 0, eid = -1;
        if ((lmask >> lane) & 1ull) {
          eid = a.loc_in_eid[lk + __popcll(lmask & lt)];
          ty = a.loc_type[eid];
        }
        const float len = ag_sqrt_rn(dist2_nofma(xi, yi, zi, spos[3 * jj], spos[3 * jj + 1], spos[3 * jj + 2]));
        a.e_loc[p] = eid >= 0 ? a.loc_row[eid] : -1;
        a.e_src[p] = g0 + j;
        a.e_dst[p] = g0 + i;
        a.e_type[p] = ty;
        a.e_len[p] = len;
        if (a.rad_cnt && eid < 0) {
          const int rp = rp0 + __popcll(rmask & lt);
          a.rad_src[rp] = g0 + j;
          a.rad_len[rp] = len;
          if (a.r_scale) {
            const float C = cf_envelope(len, a.cutoff, a.smooth);
            for (int c = 0; c < a.n_scales; ++c) a.r_scale[(size_t)c * a.rpad + rp] = cf_dist_weight(sseg + c * 100, len) * C;
          }
        }
        if (canon) {
          const int cp = cp0 + __popcll(cmask & lt);
          a.c_len[cp] = len;
          a.c_type[cp] = ty;
          a.c_src[cp] = g0 + j;
          a.c_dst[cp] = g0 + i;
          a.c_pos[cp] = p;
          a.c_mir[cp] = mir ? base + (j ? sin[j - 1] : 0) + rank_below(inbits, j, i) : -1;
        }
      }
      p0 += __popcll(emask);
      cp0 += __popcll(cmask);
      lk += __popcll(lmask);
      rp0 += __popcll(rmask);
    }
    if (a.rad_cnt) {
      const int cnt = rp0 - (g0 + i) * AGDIFF_RAD_STRIDE;
      if (lane == 0) a.rad_cnt[g0 + i] = cnt;
      if (a.r_scale && lane < ((cnt + AG_TW - 1) / AG_TW) * AG_TW - cnt) {     // pad rows: src = the target itself, length 0, scale 0
        const int rp = rp0 + lane;
        a.rad_src[rp] = g0 + i;
        a.rad_len[rp] = 0.0f;
        for (int c = 0; c < a.n_scales; ++c) a.r_scale[(size_t)c * a.rpad + rp] = 0.0f;
      }
    }
  }
  // pass 3: ref2dst, one thread per source walking its column (targets ascending = the (src, dst) order)
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    int q = base + (j ? sout[j - 1] : 0);
    const int wj = j >> 5;
    const uint32_t below = (1u << (j & 31)) - 1u;
    for (int i = 0; i < n; ++i) {
      const uint32_t* row = inbits + i * words;
      if ((row[wj] >> (j & 31)) & 1u) {
        int rank = __popc(row[wj] & below);
        for (int w = 0; w < wj; ++w) rank += __popc(row[w]);
        a.ref2dst[q++] = base + (i ? sin[i - 1] : 0) + rank;
      }
    }
  }
}

// exclusive scan of graph_edge_cnt[G] -> graph_edge_ptr[G+1]; total -> num_edges. One workgroup.
// Block 1 (if launched) does the same for the canonical counts.
__global__ void __launch_bounds__(1024) k_scan_graphs(const int32_t* __restrict__ cnt0, int32_t* __restrict__ ptr0,
                                                      int32_t* __restrict__ total0, const int32_t* __restrict__ cnt1,
                                                      int32_t* __restrict__ ptr1, int32_t* __restrict__ total1, int G) {
  const int32_t* cnt = blockIdx.x ? cnt1 : cnt0;
  int32_t* ptr = blockIdx.x ? ptr1 : ptr0;
  int32_t* total = blockIdx.x ? total1 : total0;
  __shared__ int wtot[16];
  __shared__ int carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int b0 = 0; b0 < G; b0 += 1024) {
    const int i = b0 + threadIdx.x;
    int v = (i < G) ? cnt[i] : 0;
    int s = v;
    for (int o = 1; o < 64; o <<= 1) {
      int u = __shfl_up(s, o);
      if (lane >= o) s += u;
    }
    if (lane == 63) wtot[wv] = s;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wv; ++w) woff += wtot[w];
    const int carry = carry_s;
    if (i < G) ptr[i] = carry + woff + s - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = carry + woff + s;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ptr[G] = carry_s;
    *total = carry_s;
  }
}

// one evaluation per canonical local edge (|p_i - p_j| is the same number for j -> i and i -> j: the differences only
// change sign before they are squared)
__global__ void k_local_lengths(const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                const int32_t* __restrict__ cpos, const int32_t* __restrict__ cmir,
                                const float* __restrict__ pos, float* __restrict__ len, float* __restrict__ clen, int Lc,
                                const int32_t* __restrict__ inpos, const int32_t* __restrict__ inmir,
                                float* __restrict__ len_in, const int32_t* __restrict__ tpos,
                                const int32_t* __restrict__ tmir, float* __restrict__ len_t) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Lc) return;
  int s = src[c], d = dst[c];
  const float v = ag_sqrt_rn(dist2_nofma(pos[3 * s], pos[3 * s + 1], pos[3 * s + 2], pos[3 * d], pos[3 * d + 1], pos[3 * d + 2]));
  clen[c] = v;
  len[cpos[c]] = v;
  if (cmir[c] >= 0) len[cmir[c]] = v;
  if (len_in) {          // the same by padded-list position (agdiff_topo_t.lp_*)
    len_in[inpos[c]] = v;
    if (inmir[c] >= 0) len_in[inmir[c]] = v;
  }
  if (len_t) {           // ... and by quad-tile row (agdiff_topo_t.lt_*)
    len_t[tpos[c]] = v;
    if (tmir[c] >= 0) len_t[tmir[c]] = v;
  }
}


// ------------------------------------------------------------------------------------------------------------------------
// The same graph for molecules of ANY size (agdiff_graph_build_large): no adjacency is stored, in LDS or anywhere else.
// One integer per atom replaces a mask row: thr[i] = index (inside the molecule) of target i's 33rd in-range candidate, or
// INT_MAX when it has fewer.  The radius edge j -> i then exists iff d2(i, j) < r^2 and j <= thr[i] and j != i, and d2 is
// symmetric bit for bit ((a - b)^2 == (b - a)^2), so both a target's row (its in-edges, and for each the mirror test "does
// i -> j exist") and a source's column (its out-edges: out-degree, ref2dst) are decided from positions + thr[] + the static
// local lists (in-list of i: loc_in_ptr / loc_in_eid / loc_src, sources ascending; out-list of i: the local edges
// [loc_out_ptr[i], loc_out_ptr[i + 1]), targets ascending), which the walk follows with two cursors.
//
// Grid: the ATOMS of the batch in blocks of AG_LG_TARGETS, whatever molecule they belong to (a wave finds its atom's molecule
// by bisection of graph_ptr), one wave per atom at a time, 64 candidates per ballot: a 4096-atom molecule is spread over 256
// workgroups.  Positions are read from global memory, not staged in LDS: a workgroup's atoms may belong to several
// molecules, a molecule's block (12 B per atom, 48 KB at 4096 atoms) stays in L2 while its workgroups run, and the 64 lanes
// of a chunk read 768 consecutive bytes.
// Launches: thr -> degrees (row walk: in / canonical, column walk: out) -> exclusive scans over ALL atoms (in_ptr, out_ptr
// and the canonical offsets are plain prefix sums in atom order: no per-molecule base, no atomics, nothing depends on the
// order in which workgroups arrive) -> fill (row walk again) -> ref2dst and the mirrors' positions (column walk + bisection
// of the finished in-lists).  Scratch: ws->g_deg holds thr[], ws->g_cdeg the canonical degrees and then their scan.
#define AG_LG_THREADS 256
#define AG_LG_TARGETS 16
#define AG_LG_NO_THR 0x7fffffff
#define AG_LG_MIRROR_PENDING (-2)

struct LargeArgs {
  GraphArgs g;
  const int32_t* loc_out_ptr;
  const int32_t* loc_dst;
  int32_t* thr;        // [N] ws->g_deg
  int32_t* cscan;      // [N] ws->g_cdeg
  int32_t* num_edges;
  int32_t* num_canon;
  int32_t num_nodes;
  int32_t max_edges;
};

__device__ __forceinline__ int lg_graph_of(const int32_t* __restrict__ gp, int G, int node) {
  int lo = 0, hi = G;                       // gp[lo] <= node < gp[hi]; empty graphs (gp[g] == gp[g + 1]) are stepped over
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (gp[mid] <= node) lo = mid; else hi = mid;
  }
  return lo;
}

// position of source `key` in the finished in-list [lo, hi) of a target (sources ascending; the edge exists)
__device__ __forceinline__ int lg_find(const int32_t* __restrict__ e_src, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e_src[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(AG_LG_THREADS) k_lg_thr(LargeArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int t = wave; t < AG_LG_TARGETS; t += AG_LG_THREADS / 64) {
    const int gi = blockIdx.x * AG_LG_TARGETS + t;
    if (gi >= a.num_nodes) break;
    const int g = lg_graph_of(a.g.graph_ptr, a.g.num_graphs, gi);
    const int g0 = a.g.graph_ptr[g], n = a.g.graph_ptr[g + 1] - g0;
    const float xi = a.g.pos[3 * (size_t)gi], yi = a.g.pos[3 * (size_t)gi + 1], zi = a.g.pos[3 * (size_t)gi + 2];
    int cnt = 0, thr = AG_LG_NO_THR;
    for (int c = 0; 64 * c < n; ++c) {
      const int j = 64 * c + lane;
      const bool valid = j < n;
      const size_t jj = (size_t)g0 + (valid ? j : 0);
      const float d2 = dist2_nofma(xi, yi, zi, a.g.pos[3 * jj], a.g.pos[3 * jj + 1], a.g.pos[3 * jj + 2]);
      const bool within = valid && d2 < a.g.r2;
      const uint64_t wmask = __ballot(within);
      if (cnt + __popcll(wmask) >= AGDIFF_RADIUS_CAP) {
        const uint64_t hit = __ballot(within && cnt + __popcll(wmask & lt) == AGDIFF_RADIUS_CAP - 1);
        thr = 64 * c + __builtin_ctzll(hit);
        break;
      }
      cnt += __popcll(wmask);
    }
    if (lane == 0) a.thr[gi] = thr;
  }
}

// The column of source atom gs (lanes = targets, ascending): OUT-degree, and with REF the (src, dst)-order permutation.
template <bool REF>
__device__ __forceinline__ int lg_column(const LargeArgs& a, int gs, int g0, int n, int lane, uint64_t lt) {
  const int s = gs - g0;
  const float xs = a.g.pos[3 * (size_t)gs], ys = a.g.pos[3 * (size_t)gs + 1], zs = a.g.pos[3 * (size_t)gs + 2];
  int ok = a.loc_out_ptr[gs];
  const int ok1 = a.loc_out_ptr[gs + 1];
  int q0 = REF ? a.g.out_ptr[gs] : 0, outdeg = 0;
  // (the cursor's next entry is kept in a register: a chunk without local entries then costs no dependent load)
  int next_d = ok < ok1 ? a.loc_dst[ok] - g0 : AG_LG_NO_THR;
  for (int c = 0; 64 * c < n; ++c) {
    uint64_t omask = 0;
    while (next_d < 64 * (c + 1)) {
      omask |= 1ull << (next_d - 64 * c);
      ++ok;
      next_d = ok < ok1 ? a.loc_dst[ok] - g0 : AG_LG_NO_THR;
    }
    const int i = 64 * c + lane;
    const bool valid = i < n;
    const size_t ii = (size_t)g0 + (valid ? i : 0);
    const float d2 = dist2_nofma(a.g.pos[3 * ii], a.g.pos[3 * ii + 1], a.g.pos[3 * ii + 2], xs, ys, zs);
    const bool rad = valid && d2 < a.g.r2 && i != s && s <= a.thr[ii];
    const bool e = rad || ((omask >> lane) & 1ull);
    const uint64_t xmask = __ballot(e);
    if (REF && e) {
      const int q = q0 + __popcll(xmask & lt);
      if (q < a.max_edges) a.g.ref2dst[q] = lg_find(a.g.e_src, a.g.in_ptr[ii], a.g.in_ptr[ii + 1], gs);
    }
    q0 += __popcll(xmask);
    outdeg += __popcll(xmask);
  }
  return outdeg;
}

// The row of target atom gi (lanes = candidate sources, ascending): in-degree and canonical in-degree; with FILL the lists.
template <bool FILL>
__device__ __forceinline__ void lg_row(const LargeArgs& a, const float* sseg, int gi, int g0, int n, int lane, uint64_t lt,
                                       int& deg_out, int& cdeg_out) {
  const int i = gi - g0;
  const float xi = a.g.pos[3 * (size_t)gi], yi = a.g.pos[3 * (size_t)gi + 1], zi = a.g.pos[3 * (size_t)gi + 2];
  const int thr_i = a.thr[gi];
  int lk = a.g.loc_in_ptr[gi], ok = a.loc_out_ptr[gi];
  const int lk1 = a.g.loc_in_ptr[gi + 1], ok1 = a.loc_out_ptr[gi + 1];
  // candidates beyond both the threshold and the last local source cannot be edges
  const int last_loc = lk1 > lk ? a.g.loc_src[a.g.loc_in_eid[lk1 - 1]] - g0 : -1;
  const int upper = max(min(thr_i, n - 1), last_loc);
  int p0 = FILL ? a.g.in_ptr[gi] : 0, cp0 = FILL ? a.cscan[gi] : 0;
  int rp0 = gi * AGDIFF_RAD_STRIDE;
  int deg = 0, cdeg = 0;
  // (both cursors' next entries are kept in registers: a chunk without local entries costs no dependent load)
  int next_s = lk < lk1 ? a.g.loc_src[a.g.loc_in_eid[lk]] - g0 : AG_LG_NO_THR;
  int next_d = ok < ok1 ? a.loc_dst[ok] - g0 : AG_LG_NO_THR;
  for (int c = 0; 64 * c <= upper; ++c) {
    uint64_t lmask = 0, omask = 0;
    int nk = lk;
    while (next_s < 64 * (c + 1)) {
      lmask |= 1ull << (next_s - 64 * c);
      ++nk;
      next_s = nk < lk1 ? a.g.loc_src[a.g.loc_in_eid[nk]] - g0 : AG_LG_NO_THR;
    }
    int no = ok;
    while (next_d < 64 * (c + 1)) {
      omask |= 1ull << (next_d - 64 * c);
      ++no;
      next_d = no < ok1 ? a.loc_dst[no] - g0 : AG_LG_NO_THR;
    }
    const int j = 64 * c + lane;
    const bool valid = j < n;
    const size_t jj = (size_t)g0 + (valid ? j : 0);
    const float d2 = dist2_nofma(xi, yi, zi, a.g.pos[3 * jj], a.g.pos[3 * jj + 1], a.g.pos[3 * jj + 2]);
    const bool within = valid && d2 < a.g.r2 && j != i;
    const bool lin = (lmask >> lane) & 1ull, lout = (omask >> lane) & 1ull;
    const bool e = lin || (within && j <= thr_i);
    const uint64_t emask = __ballot(e);
    const uint64_t rmask = emask & ~lmask;
    // the edge the other way round, i -> j
    const bool rout = e && within && i <= a.thr[jj];
    int ty = 0, eid = -1;
    if (lin) {
      eid = a.g.loc_in_eid[lk + __popcll(lmask & lt)];
      ty = a.g.loc_type[eid];
    }
    bool mir, canon;
    if (a.g.canon_radius_only) {
      const bool rad = e && !lin;
      mir = rad && rout && !lout;
      canon = rad && (j < i || !mir);
    } else {
      mir = e && (rout || lout) && lin == lout && (!lin || ty == a.g.loc_type[ok + __popcll(omask & lt)]);
      canon = e && (j < i || !mir);
    }
    const uint64_t cmask = __ballot(canon);
    if (FILL && e) {
      const int p = p0 + __popcll(emask & lt);
      const float len = ag_sqrt_rn(d2);
      if (p < a.max_edges) {
        a.g.e_loc[p] = eid >= 0 ? a.g.loc_row[eid] : -1;
        a.g.e_src[p] = g0 + j;
        a.g.e_dst[p] = gi;
        a.g.e_type[p] = ty;
        a.g.e_len[p] = len;
      }
      if (a.g.rad_cnt && eid < 0) {
        const int rp = rp0 + __popcll(rmask & lt);
        a.g.rad_src[rp] = g0 + j;
        a.g.rad_len[rp] = len;
        if (a.g.r_scale) {
          const float C = cf_envelope(len, a.g.cutoff, a.g.smooth);
          for (int cc = 0; cc < a.g.n_scales; ++cc) a.g.r_scale[(size_t)cc * a.g.rpad + rp] = cf_dist_weight(sseg + cc * 100, len) * C;
        }
      }
      if (canon) {
        const int cp = cp0 + __popcll(cmask & lt);
        if (cp < a.max_edges) {
          a.g.c_len[cp] = len;
          a.g.c_type[cp] = ty;
          a.g.c_src[cp] = g0 + j;
          a.g.c_dst[cp] = gi;
          a.g.c_pos[cp] = p;
          a.g.c_mir[cp] = mir ? AG_LG_MIRROR_PENDING : -1;      // (k_lg_ref looks the position up once every list is written)
        }
      }
    }
    p0 += __popcll(emask);
    cp0 += __popcll(cmask);
    rp0 += __popcll(rmask);
    deg += __popcll(emask);
    cdeg += __popcll(cmask);
    lk = nk;
    ok = no;
  }
  if (FILL && a.g.rad_cnt) {
    const int cnt = rp0 - gi * AGDIFF_RAD_STRIDE;
    if (lane == 0) a.g.rad_cnt[gi] = cnt;
    if (a.g.r_scale && lane < ((cnt + AG_TW - 1) / AG_TW) * AG_TW - cnt) {     // pad rows, as k_graph writes them
      const int rp = rp0 + lane;
      a.g.rad_src[rp] = gi;
      a.g.rad_len[rp] = 0.0f;
      for (int cc = 0; cc < a.g.n_scales; ++cc) a.g.r_scale[(size_t)cc * a.g.rpad + rp] = 0.0f;
    }
  }
  deg_out = deg;
  cdeg_out = cdeg;
}

__global__ void __launch_bounds__(AG_LG_THREADS) k_lg_count(LargeArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int t = wave; t < AG_LG_TARGETS; t += AG_LG_THREADS / 64) {
    const int gi = blockIdx.x * AG_LG_TARGETS + t;
    if (gi >= a.num_nodes) break;
    const int g = lg_graph_of(a.g.graph_ptr, a.g.num_graphs, gi);
    const int g0 = a.g.graph_ptr[g], n = a.g.graph_ptr[g + 1] - g0;
    int deg, cdeg;
    lg_row<false>(a, nullptr, gi, g0, n, lane, lt, deg, cdeg);
    const int outdeg = lg_column<false>(a, gi, g0, n, lane, lt);
    if (lane == 0) {            // counts now, offsets after k_lg_scan
      a.g.in_ptr[gi] = deg;
      a.g.out_ptr[gi] = outdeg;
      a.cscan[gi] = cdeg;
    }
  }
}

// Exclusive scans over all N atoms, in place: block 0 in-degrees -> in_ptr[N + 1] (total -> num_edges), block 1 out-degrees ->
// out_ptr[N + 1], block 2 canonical degrees -> cscan[N] (total -> num_canon).  Every thread owns a run of consecutive atoms.
__global__ void __launch_bounds__(1024) k_lg_scan(LargeArgs a) {
  int32_t* arr = blockIdx.x == 0 ? a.g.in_ptr : blockIdx.x == 1 ? a.g.out_ptr : a.cscan;
  const int N = a.num_nodes;
  const int per = (N + 1023) / 1024;
  const int lo = min((int)threadIdx.x * per, N), hi = min(lo + per, N);
  int sum = 0;
  for (int k = lo; k < hi; ++k) sum += arr[k];
  __shared__ int wtot[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int s = sum;
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(s, o);
    if (lane >= o) s += u;
  }
  if (lane == 63) wtot[wv] = s;
  __syncthreads();
  int run = s - sum;
  for (int w = 0; w < wv; ++w) run += wtot[w];
  for (int k = lo; k < hi; ++k) {
    const int v = arr[k];
    arr[k] = run;
    run += v;
  }
  if (threadIdx.x == 1023) {
    if (blockIdx.x < 2) arr[N] = run;
    if (blockIdx.x == 0) *a.num_edges = run;
    if (blockIdx.x == 2) *a.num_canon = run;
  }
}

__global__ void __launch_bounds__(AG_LG_THREADS) k_lg_fill(LargeArgs a) {
  __shared__ float sseg[2 * AGDIFF_MAX_CONVS * 100];
  if (a.g.r_scale) {
    for (int i = threadIdx.x; i < a.g.n_scales * 100; i += blockDim.x) sseg[i] = a.g.dw[i / 100][i % 100];
    __syncthreads();
  }
  // the per-molecule views of the scans
  const int N = a.num_nodes, G = a.g.num_graphs;
  for (int g = blockIdx.x * AG_LG_THREADS + threadIdx.x; g <= G; g += gridDim.x * AG_LG_THREADS) {
    const int n0 = a.g.graph_ptr[g];
    const int e0 = a.g.in_ptr[n0], c0 = n0 < N ? a.cscan[n0] : *a.num_canon;
    const_cast<int32_t*>(a.g.graph_edge_ptr)[g] = e0;
    const_cast<int32_t*>(a.g.graph_canon_ptr)[g] = c0;
    if (g < G) {
      const int n1 = a.g.graph_ptr[g + 1];
      a.g.graph_edge_cnt[g] = a.g.in_ptr[n1] - e0;
      a.g.graph_canon_cnt[g] = (n1 < N ? a.cscan[n1] : *a.num_canon) - c0;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int t = wave; t < AG_LG_TARGETS; t += AG_LG_THREADS / 64) {
    const int gi = blockIdx.x * AG_LG_TARGETS + t;
    if (gi >= N) break;
    const int g = lg_graph_of(a.g.graph_ptr, G, gi);
    const int g0 = a.g.graph_ptr[g], n = a.g.graph_ptr[g + 1] - g0;
    int deg, cdeg;
    lg_row<true>(a, sseg, gi, g0, n, lane, lt, deg, cdeg);
  }
}

__global__ void __launch_bounds__(AG_LG_THREADS) k_lg_ref(LargeArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const int N = a.num_nodes;
  for (int t = wave; t < AG_LG_TARGETS; t += AG_LG_THREADS / 64) {
    const int gi = blockIdx.x * AG_LG_TARGETS + t;
    if (gi >= N) break;
    const int g = lg_graph_of(a.g.graph_ptr, a.g.num_graphs, gi);
    const int g0 = a.g.graph_ptr[g], n = a.g.graph_ptr[g + 1] - g0;
    lg_column<true>(a, gi, g0, n, lane, lt);
  }
  // the canonical entries of this block's targets: the mirror i -> j of the canonical edge j -> i sits in j's in-list
  const int a0 = blockIdx.x * AG_LG_TARGETS, a1 = min(a0 + AG_LG_TARGETS, N);
  const int c0 = a.cscan[a0], c1 = min(a1 < N ? a.cscan[a1] : *a.num_canon, a.max_edges);
  for (int cp = c0 + (int)threadIdx.x; cp < c1; cp += AG_LG_THREADS)
    if (a.g.c_mir[cp] == AG_LG_MIRROR_PENDING) {
      const int j = a.g.c_src[cp];
      a.g.c_mir[cp] = lg_find(a.g.e_src, a.g.in_ptr[j], a.g.in_ptr[j + 1], a.g.c_dst[cp]);
    }
}

}  // namespace

extern "C" int agdiff_graph_build(const agdiff_topo_t* topo, const agdiff_ws_t* ws, const float* pos, float cutoff,
                                  void* stream) {
  return agdiff_graph_build_ex(topo, ws, pos, cutoff, 0, stream);
}

namespace {
int graph_build_impl(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, const float* pos, float cutoff,
                     int32_t canon_radius_only, void* stream, bool force_large = false);
}

extern "C" int agdiff_graph_build_ex(const agdiff_topo_t* topo, const agdiff_ws_t* ws, const float* pos, float cutoff,
                                     int32_t canon_radius_only, void* stream) {
  return graph_build_impl(nullptr, topo, ws, pos, cutoff, canon_radius_only, stream);
}

extern "C" int agdiff_graph_build_scaled(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws,
                                         const float* pos, float cutoff, int32_t canon_radius_only, void* stream) {
  if (!p || !ws || !ws->r_scale || !ws->rad_cnt || p->num_convs > AGDIFF_MAX_CONVS) return AGDIFF_ERR_ARG;
  return graph_build_impl(p, topo, ws, pos, cutoff, canon_radius_only, stream);
}

extern "C" int agdiff_graph_build_large(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws,
                                        const float* pos, float cutoff, int32_t canon_radius_only, void* stream) {
  if (p && (!ws || !ws->r_scale || !ws->rad_cnt || p->num_convs > AGDIFF_MAX_CONVS)) return AGDIFF_ERR_ARG;
  return graph_build_impl(p, topo, ws, pos, cutoff, canon_radius_only, stream, true);
}

extern "C" int agdiff_graph_large_grid(const agdiff_topo_t* topo, int64_t* out) {
  if (!topo || !out || topo->num_nodes <= 0) return AGDIFF_ERR_ARG;
  out[0] = (topo->num_nodes + AG_LG_TARGETS - 1) / AG_LG_TARGETS;
  out[1] = AG_LG_TARGETS;
  return AGDIFF_OK;
}

namespace {
// agdiff_graph_build_large's five launches (`a` filled by graph_build_impl)
int graph_build_large(const GraphArgs& ga, const agdiff_topo_t* topo, const agdiff_ws_t* ws, hipStream_t st) {
  if (!ws->g_deg || !ws->g_cdeg || !topo->loc_out_ptr || !topo->loc_in_ptr || (topo->num_local > 0 && (!topo->loc_dst || !topo->loc_src ||
      !topo->loc_in_eid || !topo->loc_type)))
    return AGDIFF_ERR_ARG;
  if (topo->num_nodes * (int64_t)AGDIFF_RAD_STRIDE >= (1ll << 31) || topo->max_edges >= (1ll << 31)) return AGDIFF_ERR_LIMIT;
  LargeArgs a;
  a.g = ga;
  a.loc_out_ptr = topo->loc_out_ptr;
  a.loc_dst = topo->loc_dst;
  a.thr = ws->g_deg;
  a.cscan = ws->g_cdeg;
  a.num_edges = ws->num_edges;
  a.num_canon = ws->num_canon;
  a.num_nodes = (int32_t)topo->num_nodes;
  a.max_edges = (int32_t)topo->max_edges;
  const unsigned blocks = (unsigned)((topo->num_nodes + AG_LG_TARGETS - 1) / AG_LG_TARGETS);
  ag_log_variant(ws, AGDIFF_VAR_GRAPH_LARGE);
  k_lg_thr<<<blocks, AG_LG_THREADS, 0, st>>>(a);
  AG_CHECK_LAUNCH();
  k_lg_count<<<blocks, AG_LG_THREADS, 0, st>>>(a);
  AG_CHECK_LAUNCH();
  k_lg_scan<<<3, 1024, 0, st>>>(a);
  AG_CHECK_LAUNCH();
  k_lg_fill<<<blocks, AG_LG_THREADS, 0, st>>>(a);
  AG_CHECK_LAUNCH();
  k_lg_ref<<<blocks, AG_LG_THREADS, 0, st>>>(a);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

int graph_build_impl(const agdiff_params_t* p, const agdiff_topo_t* topo, const agdiff_ws_t* ws, const float* pos, float cutoff,
                     int32_t canon_radius_only, void* stream, bool force_large) {
  if (!topo || !ws || !pos || topo->num_graphs <= 0 || topo->num_nodes <= 0 || (topo->num_local > 0 && !topo->loc_row))
    return AGDIFF_ERR_ARG;
  if (!ws->graph_edge_cnt || !ws->graph_edge_ptr || !ws->in_ptr || !ws->out_ptr || !ws->e_src || !ws->e_dst ||
      !ws->e_type || !ws->e_len || !ws->ref2dst || !ws->e_loc || !ws->num_edges || !ws->num_canon ||
      !ws->graph_canon_cnt || !ws->graph_canon_ptr || !ws->c_len || !ws->c_type || !ws->c_src || !ws->c_dst ||
      !ws->c_pos || !ws->c_mir)
    return AGDIFF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  // Up to AGDIFF_MAX_ATOMS_PER_GRAPH atoms per molecule: k_graph, LDS sized for the word count the batch's largest molecule
  // needs.  Beyond (up to AGDIFF_MAX_ATOMS_LARGE): the k_lg_* kernels.
  GraphArgs a;
  a.graph_ptr = topo->graph_ptr;
  a.loc_in_ptr = topo->loc_in_ptr;
  a.loc_in_eid = topo->loc_in_eid;
  a.loc_src = topo->loc_src;
  a.loc_type = topo->loc_type;
  a.loc_row = topo->loc_row;
  a.pos = pos;
  a.r2 = cutoff * cutoff;
  a.graph_edge_cnt = ws->graph_edge_cnt;
  a.graph_edge_ptr = ws->graph_edge_ptr;
  a.in_ptr = ws->in_ptr;
  a.out_ptr = ws->out_ptr;
  a.e_src = ws->e_src;
  a.e_dst = ws->e_dst;
  a.e_type = ws->e_type;
  a.e_len = ws->e_len;
  a.ref2dst = ws->ref2dst;
  a.e_loc = ws->e_loc;
  a.graph_canon_cnt = ws->graph_canon_cnt;
  a.graph_canon_ptr = ws->graph_canon_ptr;
  a.c_len = ws->c_len;
  a.c_type = ws->c_type;
  a.c_src = ws->c_src;
  a.c_dst = ws->c_dst;
  a.c_pos = ws->c_pos;
  a.c_mir = ws->c_mir;
  const bool rad = ws->rad_cnt && ws->rad_src && ws->rad_len;
  a.rad_cnt = rad ? ws->rad_cnt : nullptr;
  a.rad_src = ws->rad_src;
  a.rad_len = ws->rad_len;
  if (canon_radius_only && !rad) return AGDIFF_ERR_ARG;
  a.canon_radius_only = canon_radius_only ? 1 : 0;
  const bool handover = ws->g_inbits && ws->g_deg && ws->g_cdeg;
  a.g_inbits = handover ? reinterpret_cast<uint32_t*>(ws->g_inbits) : nullptr;
  a.g_deg = ws->g_deg;
  a.g_cdeg = ws->g_cdeg;
  a.num_graphs = (int32_t)topo->num_graphs;
  a.r_scale = nullptr;
  a.rpad = 0;
  a.n_scales = 0;
  a.cutoff = cutoff;
  a.smooth = 0;
  if (p) {                 // the radius rows' CFConv scales from the fill pass (agdiff_graph_build_scaled)
    for (int k = 0; k < p->num_convs; ++k) {
      a.dw[2 * k] = p->conv[k].dist_seg;
      a.dw[2 * k + 1] = p->conv[k].dist_seg + 100;
    }
    a.r_scale = ws->r_scale;
    a.rpad = topo->num_nodes * (int64_t)AGDIFF_RAD_STRIDE;
    a.n_scales = 2 * p->num_convs;
    a.cutoff = p->cutoff;       // (the envelope's cutoff is the model's, also when the graph is built without radius edges)
    a.smooth = p->smooth;
  }
  const int max_atoms = (int)topo->max_atoms_per_graph;
  if (max_atoms <= 0 || max_atoms > AGDIFF_MAX_ATOMS_LARGE) return AGDIFF_ERR_LIMIT;
  // molecules past the LDS path's limit (and agdiff_graph_build_large on any batch): the mask-free build
  a.words = 0;
  if (force_large || max_atoms > AGDIFF_MAX_ATOMS_PER_GRAPH) return graph_build_large(a, topo, ws, st);
  a.words = 2 * ((max_atoms + 63) / 64);
  const int nmax = a.words * 32;
  // threads per molecule: a wave walks its targets one after the other (per target a chain of ballots and dependent
  // look-ups), so more waves per molecule shorten the launch until the workgroups no longer fit the chip at once
  // (1 x 100 conformers: 61 / 45 / 37 us with 256 / 512 / 1024 threads; 1024 molecules: 133 / 119 / 123)
  const int bd = topo->num_graphs >= 512 ? 512 : 1024;
  const size_t smem = (size_t)(3 * nmax + 3 * nmax + 2 * nmax * a.words) * 4;
  if (smem > 48 * 1024) {       // (molecules of more than 384 atoms)
    // the attribute is the most this launcher ever asks for (AGDIFF_MAX_ATOMS_PER_GRAPH atoms), not all 160 KiB of a CU: dynamic
    // plus static LDS (k_graph<true>'s segment tables, 6.4 KB) must fit 160 KiB, or the runtime refuses the attribute
    constexpr int wmax = 2 * ((AGDIFF_MAX_ATOMS_PER_GRAPH + 63) / 64), nbig = wmax * 32;
    constexpr size_t smem_max = (size_t)(3 * nbig + 3 * nbig + 2 * nbig * wmax) * 4;
    static_assert(smem_max + 8 * 1024 <= 160 * 1024, "k_graph's LDS at AGDIFF_MAX_ATOMS_PER_GRAPH");
    static std::atomic<uint64_t> attr_done{0};
    if (!ag_allow_big_lds(attr_done, smem_max, k_graph<false>, k_graph<true>)) return AGDIFF_ERR_LAUNCH;
  }
  k_graph<false><<<dim3((unsigned)topo->num_graphs), dim3(bd), smem, st>>>(a);
  AG_CHECK_LAUNCH();
  k_scan_graphs<<<2, 1024, 0, st>>>(ws->graph_edge_cnt, ws->graph_edge_ptr, ws->num_edges, ws->graph_canon_cnt,
                                    ws->graph_canon_ptr, ws->num_canon, (int)topo->num_graphs);
  AG_CHECK_LAUNCH();
  k_graph<true><<<dim3((unsigned)topo->num_graphs), dim3(bd), smem, st>>>(a);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}
}  // namespace

extern "C" int agdiff_local_lengths(const agdiff_topo_t* topo, const agdiff_ws_t* ws, const float* pos, void* stream) {
  if (!topo || !ws || !pos || !ws->l_len || !ws->lc_len) return AGDIFF_ERR_ARG;
  if (topo->num_local == 0) return AGDIFF_OK;
  if (!topo->lc_src || !topo->lc_dst || !topo->lc_pos || !topo->lc_mir || topo->num_local_canon <= 0) return AGDIFF_ERR_ARG;
  const int Lc = (int)topo->num_local_canon;
  const bool by_slot = ws->l_len_p && topo->lc_ppos && topo->lc_pmir;
  const bool by_tile = ws->lt_len && topo->lc_tpos && topo->lc_tmir;
  k_local_lengths<<<(Lc + 255) / 256, 256, 0, (hipStream_t)stream>>>(topo->lc_src, topo->lc_dst, topo->lc_pos, topo->lc_mir,
                                                                     pos, ws->l_len, ws->lc_len, Lc, topo->lc_ppos,
                                                                     topo->lc_pmir, by_slot ? ws->l_len_p : nullptr,
                                                                     topo->lc_tpos, topo->lc_tmir, by_tile ? ws->lt_len : nullptr);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}
