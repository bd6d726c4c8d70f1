// Evaluation kernels: the RMSD confusion matrix of get_rmsd_confusion_matrix
// (utils/evaluation/covmat.py:16-35) and its row / column minima (covmat.py:135-136).
//
// rdkit's GetBestRMS (third party, not vendored by the reference) = min over the molecule's self-matches of the RMSD
// after AlignMol's optimal proper rotation + translation.  For one mapping, with both conformers centred,
//   RMSD^2 = (|X|^2 + |Y|^2 - 2 lambda_max(K)) / m,
// K = Horn's 4x4 symmetric key matrix of the 3x3 cross-covariance S = sum_k x_k y_k^T (largest eigenvalue = the best
// proper rotation as a unit quaternion; reflections are excluded by construction).  lambda_max comes from cyclic
// Jacobi sweeps in fp64: a few hundred flops per pair, robust for planar / collinear / identical conformers.
// Latency-bound, tiny next to the sampler: one thread per (reference, generated) pair, conformer tiles staged in LDS.
//
// There is ONE copy of each step of that formula: ag_cov_add (S), ag_horn_key (K), ag_jacobi4 (the sweeps, with or without
// eigenvectors) and ag_pair_msd (the minimum over the mappings, with or without the mirror image).  k_rmsd_matrix<false>,
// k_rmsd_matrix<true> and k_rmsd_self agree bit for bit because they call that one routine; k_align_conformers runs the same sweeps.
#include "common.hpp"

namespace {

// each argument summed over the 64 lanes of the wave, in place, in every lane: xor butterfly, offsets 32, 16, ... 1
template <typename... T>
__device__ __forceinline__ void ag_wave_sum(T&... x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ((x += __shfl_xor(x, o)), ...);
}
template <int N>
__device__ __forceinline__ void ag_wave_sum(double (&x)[N]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] += __shfl_xor(x[e], o);
}

// every listed atom index lies in [0, n)
template <typename... I>
__device__ __forceinline__ bool ag_atoms_in_range(int n, I... a) {
  return (((unsigned)a < (unsigned)n) && ...);
}

// the atoms [a0, a1) of graph g of a packed batch of N atoms: the walk of the one-wave-per-graph kernels is
// for (a = a0 + lane; a < a1; a += 64).  Clamped to [0, N]: a graph_ptr that is not one touches nothing outside.
__device__ __forceinline__ void ag_graph_span(const int32_t* __restrict__ graph_ptr, int g, int N, int& a0, int& a1) {
  a0 = max(graph_ptr[g], 0);
  a1 = min(graph_ptr[g + 1], N);
}

// neither Inf nor NaN
__device__ __forceinline__ bool ag_finite(double x) { return fabs(x) <= 1.79769313486231570e308; }

// centred coordinates of the selected atoms, one wave per conformer (centroid in fp64, rounded once):
// out[c] = { x_0 y_0 z_0 ... x_{m-1} y_{m-1} z_{m-1} | unused }
__global__ void __launch_bounds__(64) k_center_selected(const float* __restrict__ pos, const int32_t* __restrict__ idx,
                                                        int n, int m, float* __restrict__ out) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const float* p = pos + (size_t)c * n * 3;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int k = lane; k < m; k += 64) {
    const int a = idx[k];
    sx += p[3 * a]; sy += p[3 * a + 1]; sz += p[3 * a + 2];
  }
  ag_wave_sum(sx, sy, sz);
  const double cx = sx / m, cy = sy / m, cz = sz / m;
  float* o = out + (size_t)c * (3 * m + 1);
  for (int k = lane; k < m; k += 64) {
    const int a = idx[k];
    o[3 * k] = (float)(p[3 * a] - cx); o[3 * k + 1] = (float)(p[3 * a + 1] - cy); o[3 * k + 2] = (float)(p[3 * a + 2] - cz);
  }
  if (lane == 0) o[3 * m] = 0.0f;
}

// cross-covariance of one atom pair: S += x y^T, row-major
__device__ __forceinline__ void ag_cov_add(double (&S)[9], double x0, double x1, double x2, double y0, double y1, double y2) {
  S[0] += x0 * y0; S[1] += x0 * y1; S[2] += x0 * y2;
  S[3] += x1 * y0; S[4] += x1 * y1; S[5] += x1 * y2;
  S[6] += x2 * y0; S[7] += x2 * y1; S[8] += x2 * y2;
}

// Horn's key matrix of the cross-covariance S: the upper triangle K[0..9] = (00 01 02 03 11 12 13 22 23 33) of a symmetric 4x4
__device__ __forceinline__ void ag_horn_key(const double (&S)[9], double (&K)[10]) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  K[0] = Sxx + Syy + Szz; K[1] = Syz - Szy; K[2] = Szx - Sxz; K[3] = Sxy - Syx;
  K[4] = Sxx - Syy - Szz; K[5] = Sxy + Syx; K[6] = Szx + Sxz;
  K[7] = -Sxx + Syy - Szz; K[8] = Syz + Szy;
  K[9] = -Sxx - Syy + Szz;
}

// cyclic Jacobi sweeps over the symmetric 4x4 matrix with upper triangle k (12 at most, until the off-diagonal mass is gone):
// d = the diagonal that is left, the eigenvalues in no particular order; kVectors: vectors = the accumulated rotations, column j
// the eigenvector of d[j] (not touched otherwise).  A and V are locals and the results are copied out at the end: a matrix
// handed in by reference stays in memory until this is inlined, and the unrolled sweeps then compile to other code.
template <bool kVectors>
__device__ void ag_jacobi4(const double (&k)[10], double (&d)[4], double (*vectors)[4] = nullptr) {
  double A[4][4] = {{k[0], k[1], k[2], k[3]}, {k[1], k[4], k[5], k[6]}, {k[2], k[5], k[7], k[8]}, {k[3], k[6], k[8], k[9]}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 12; ++sweep) {
    double off = 0.0;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) off += A[p][q] * A[p][q];
    if (off < 1e-30) break;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {           // columns p, q
          const double arp = A[r][p], arq = A[r][q];
          A[r][p] = c * arp - s * arq;
          A[r][q] = s * arp + c * arq;
          if constexpr (kVectors) {
            const double vrp = V[r][p], vrq = V[r][q];
            V[r][p] = c * vrp - s * vrq;
            V[r][q] = s * vrp + c * vrq;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {           // rows p, q
          const double apr = A[p][r], aqr = A[q][r];
          A[p][r] = c * apr - s * aqr;
          A[q][r] = s * apr + c * aqr;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    d[r] = A[r][r];
    if constexpr (kVectors) {
#pragma unroll
      for (int c = 0; c < 4; ++c) vectors[r][c] = V[r][c];
    }
  }
}

// Mean-square deviation of the conformers x and y (centred, m atoms, 3 m floats each) after the best proper rotation, minimised
// over the P atom mappings of y (perms == nullptr: the identity alone).  kMirror: best_mirror = the same for x inverted through
// its centroid.  K is linear in S and the inversion turns S into -S, so lambda_max(K(-S)) = -lambda_min(K(S)): the best fit of
// the mirror image comes out of the diagonalisation the proper fit already pays for.
template <bool kMirror>
__device__ __forceinline__ void ag_pair_msd(const float* x, const float* y, const int32_t* perms, int m, int P, double& best,
                                            double& best_mirror) {
  // squared norms from the SAME rounded coordinates the cross-covariance uses, in fp64: near RMSD = 0 the difference
  // |X|^2 + |Y|^2 - 2 lambda cancels to ~1e-16 relative only if both sides see identical inputs
  double gsum = 0.0;
  for (int k = 0; k < m; ++k) {
    const double x0 = x[3 * k], x1 = x[3 * k + 1], x2 = x[3 * k + 2];
    const double y0 = y[3 * k], y1 = y[3 * k + 1], y2 = y[3 * k + 2];
    gsum += (x0 * x0 + x1 * x1 + x2 * x2) + (y0 * y0 + y1 * y1 + y2 * y2);
  }
  best = 1e300;
  if constexpr (kMirror) best_mirror = 1e300;
  for (int p = 0; p < (perms ? P : 1); ++p) {
    const int32_t* pm = perms ? perms + (size_t)p * m : nullptr;
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < m; ++k) {
      const int kr = pm ? pm[k] : k;
      const double x0 = x[3 * k], x1 = x[3 * k + 1], x2 = x[3 * k + 2];
      const double y0 = y[3 * kr], y1 = y[3 * kr + 1], y2 = y[3 * kr + 2];
      ag_cov_add(S, x0, x1, x2, y0, y1, y2);
    }
    double K[10], d[4];
    ag_horn_key(S, K);
    ag_jacobi4<false>(K, d);
    best = fmin(best, (gsum - 2.0 * fmax(fmax(d[0], d[1]), fmax(d[2], d[3]))) / m);
    if constexpr (kMirror) best_mirror = fmin(best_mirror, (gsum + 2.0 * fmin(fmin(d[0], d[1]), fmin(d[2], d[3]))) / m);
  }
}

extern __shared__ float ag_eval_smem[];

// two LDS tiles of 16 centred conformers each (`stride` floats per conformer): a0 .. a0 + 15 of the na conformers of a, the
// same for b; zeros past the end.  The caller synchronises.
__device__ __forceinline__ void ag_stage_tiles(float* sa, const float* a, int a0, int na, float* sb, const float* b, int b0, int nb,
                                               int stride) {
  for (int t = threadIdx.x; t < 16 * stride; t += 256) {
    const int c = t / stride, o = t % stride;
    sa[t] = (a0 + c < na) ? a[(size_t)(a0 + c) * stride + o] : 0.0f;
    sb[t] = (b0 + c < nb) ? b[(size_t)(b0 + c) * stride + o] : 0.0f;
  }
}

// 16 x 16 pairs per workgroup: thread (ty, tx) = (reference ty, generated tx) of the tile.  kMirror: out_mirror = the same quantity
// for the generated conformer inverted through its centroid, minimised over the same mappings (out_mirror is not read otherwise)
template <bool kMirror>
__global__ void __launch_bounds__(256) k_rmsd_matrix(const float* __restrict__ cref, const float* __restrict__ cgen,
                                                     const int32_t* __restrict__ perms, int R, int G, int m, int P,
                                                     float* __restrict__ out, float* __restrict__ out_mirror) {
  const int stride = 3 * m + 1;
  float* sref = ag_eval_smem;
  float* sgen = ag_eval_smem + 16 * stride;
  const int j0 = blockIdx.y * 16, i0 = blockIdx.x * 16;
  ag_stage_tiles(sref, cref, j0, R, sgen, cgen, i0, G, stride);
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  if (j0 + ty >= R || i0 + tx >= G) return;
  double best, best_mirror;
  const float* y = sref + ty * stride;      // reference
  const float* x = sgen + tx * stride;      // generated (probe)
  ag_pair_msd<kMirror>(x, y, perms, m, P, best, best_mirror);
  const size_t at = (size_t)(j0 + ty) * G + i0 + tx;
  out[at] = (float)sqrt(fmax(best, 0.0));
  if constexpr (kMirror) out_mirror[at] = (float)sqrt(fmax(best_mirror, 0.0));
}

// Trajectory tracking: the RMSD of graph g in frame s to that graph's atoms of `target`, after the best proper rotation, over the
// atoms with select[a] != 0 -- identity mapping, one wave per (g, s), lanes striding over the graph's atoms whatever their number.
// The recipe of the header above with the centring of k_center_selected folded in: centroids in fp64, centred coordinates rounded
// to fp32 once, S and the squared norms from those rounded values in fp64.  kMirror: out_mirror = the same for the frame inverted
// through its centroid, from the same diagonalisation (ag_pair_msd).  NaN when a selected coordinate of either side is not finite
// (or the centred coordinates leave fp32's range), and for a graph with no selected atom.
template <bool kMirror>
__global__ void __launch_bounds__(64) k_traj_rmsd(const float* __restrict__ frames, long long frame_stride, const float* __restrict__ target,
                                                  const uint8_t* __restrict__ select, const int32_t* __restrict__ graph_ptr, int G, int N,
                                                  float* __restrict__ out, float* __restrict__ out_mirror) {
  const int g = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  const float* p = frames + (size_t)s * frame_stride;
  int a0, a1;
  ag_graph_span(graph_ptr, g, N, a0, a1);
  double c[7] = {0, 0, 0, 0, 0, 0, 0};          // sums of the frame's and the target's selected atoms, and their number
  for (int a = a0 + lane; a < a1; a += 64) {
    if (!select[a]) continue;
    const size_t o = (size_t)3 * a;
    c[0] += p[o]; c[1] += p[o + 1]; c[2] += p[o + 2];
    c[3] += target[o]; c[4] += target[o + 1]; c[5] += target[o + 2];
    c[6] += 1.0;
  }
  ag_wave_sum(c);
  const double m = c[6];
  bool ok = m > 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) ok = ok && ag_finite(c[e]);
  double best = 0.0, best_mirror = 0.0;
  if (ok) {                                      // (wave-uniform: every lane holds the same sums)
    const double cx = c[0] / m, cy = c[1] / m, cz = c[2] / m, tx = c[3] / m, ty = c[4] / m, tz = c[5] / m;
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, gsum = 0.0;
    for (int a = a0 + lane; a < a1; a += 64) {
      if (!select[a]) continue;
      const size_t o = (size_t)3 * a;
      const double x0 = (float)(p[o] - cx), x1 = (float)(p[o + 1] - cy), x2 = (float)(p[o + 2] - cz);
      const double y0 = (float)(target[o] - tx), y1 = (float)(target[o + 1] - ty), y2 = (float)(target[o + 2] - tz);
      ag_cov_add(S, x0, x1, x2, y0, y1, y2);
      gsum += (x0 * x0 + x1 * x1 + x2 * x2) + (y0 * y0 + y1 * y1 + y2 * y2);
    }
    ag_wave_sum(S);
    ag_wave_sum(gsum);
    ok = ag_finite(gsum);
    if (ok) {
      double K[10], d[4];
      ag_horn_key(S, K);
      ag_jacobi4<false>(K, d);
      best = (gsum - 2.0 * fmax(fmax(d[0], d[1]), fmax(d[2], d[3]))) / m;
      if constexpr (kMirror) best_mirror = (gsum + 2.0 * fmin(fmin(d[0], d[1]), fmin(d[2], d[3]))) / m;
    }
  }
  if (lane == 0) {
    const float nan = __int_as_float(0x7fc00000);
    const size_t at = (size_t)s * G + g;
    out[at] = ok ? (float)sqrt(fmax(best, 0.0)) : nan;
    if constexpr (kMirror) out_mirror[at] = ok ? (float)sqrt(fmax(best_mirror, 0.0)) : nan;
  }
}

// one wave per row (blockIdx.y == 0) or per column (== 1)
__global__ void __launch_bounds__(64) k_matrix_minima(const float* __restrict__ mat, int R, int G, float* __restrict__ row_min,
                                                      float* __restrict__ col_min) {
  const int lane = threadIdx.x, i = blockIdx.x;
  float v = INFINITY;
  if (blockIdx.y == 0) {
    if (i >= R) return;
    for (int c = lane; c < G; c += 64) v = fminf(v, mat[(size_t)i * G + c]);
  } else {
    if (i >= G) return;
    for (int r = lane; r < R; r += 64) v = fminf(v, mat[(size_t)r * G + i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  if (lane == 0) (blockIdx.y == 0 ? row_min : col_min)[i] = v;
}

// ---- conformer ensembles (the step after the sampler): gen x gen RMSD over the upper triangle with a fused threshold
// bit-matrix, the greedy leader prune over that matrix, and a Kabsch alignment that writes coordinates ----------------

// tile (ti <= tj) of linear block b in the row-major walk of the upper triangle of a T x T tile grid
__device__ __forceinline__ void ag_triangle_tile(long long b, int T, int& ti, int& tj) {
  const double w = 2.0 * T + 1.0;
  int r = (int)((w - sqrt(w * w - 8.0 * (double)b)) * 0.5);
  r = r < 0 ? 0 : (r > T - 1 ? T - 1 : r);
  // first block of tile row r: r T - r (r - 1) / 2 (the square root may be one off either way)
  while (r > 0 && (long long)r * T - (long long)r * (r - 1) / 2 > b) --r;
  while (r < T - 1 && (long long)(r + 1) * T - (long long)(r + 1) * r / 2 <= b) ++r;
  ti = r;
  tj = r + (int)(b - ((long long)r * T - (long long)r * (r - 1) / 2));
}

// 16 x 16 pairs per workgroup, upper-triangular tiles only: thread (ty, tx) = (conformer i0 + ty, conformer j0 + tx),
// ag_pair_msd with x = conformer i, y = conformer j, computed once for i < j and mirrored through LDS.
// bits: rows of 16-bit pieces (piece w of row i = columns 16 w .. 16 w + 15), row pitch `pitch` bytes; every piece has ONE
// writer, the tile that owns it -- (ti, tj) writes piece tj of its rows i0.. and piece ti of the rows j0.., a diagonal tile
// its own pieces once and the zero pieces that pad its rows up to the pitch.
__global__ void __launch_bounds__(256) k_rmsd_self(const float* __restrict__ cen, const int32_t* __restrict__ perms, int G, int m,
                                                   int P, int T, float thresh, float* __restrict__ out,
                                                   uint16_t* __restrict__ bits, int pitch) {
  const int stride = 3 * m + 1;
  float* srow = ag_eval_smem;                       // conformers i0 .. i0 + 15
  float* scol = ag_eval_smem + 16 * stride;         // conformers j0 .. j0 + 15
  float* sval = ag_eval_smem + 32 * stride;         // [16][17] values, then [16][17] flags
  float* sflag = sval + 16 * 17;
  int ti, tj;
  ag_triangle_tile((long long)blockIdx.x, T, ti, tj);
  const int i0 = ti * 16, j0 = tj * 16;
  const bool diag = ti == tj;
  ag_stage_tiles(srow, cen, i0, G, scol, cen, j0, G, stride);
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const bool valid = i0 + ty < G && j0 + tx < G;
  float v = 0.0f;
  if (valid && (!diag || ty < tx)) {
    double best, unused;
    ag_pair_msd<false>(srow + ty * stride, scol + tx * stride, perms, m, P, best, unused);
    v = (float)sqrt(fmax(best, 0.0));
  }
  // the threshold is taken on the fp32 value as stored, so that bits == (out <= thresh) exactly
  const float f = (valid && v <= thresh) ? 1.0f : 0.0f;
  if (!diag || ty <= tx) { sval[ty * 17 + tx] = v; sflag[ty * 17 + tx] = f; }
  if (diag && ty < tx) { sval[tx * 17 + ty] = v; sflag[tx * 17 + ty] = f; }      // symmetrised in LDS: the tile is written once
  __syncthreads();
  if (out) {
    if (valid) out[(size_t)(i0 + ty) * G + j0 + tx] = sval[ty * 17 + tx];
    if (!diag && j0 + ty < G && i0 + tx < G) out[(size_t)(j0 + ty) * G + i0 + tx] = sval[tx * 17 + ty];
  }
  if (bits) {
    const int t = threadIdx.x;
    if (t < 16) {                                   // piece tj of row i0 + t
      if (i0 + t < G) {
        unsigned w = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) w |= (sflag[t * 17 + c] != 0.0f ? 1u : 0u) << c;
        bits[(size_t)(i0 + t) * (pitch >> 1) + tj] = (uint16_t)w;
      }
    } else if (t < 32) {                            // piece ti of row j0 + (t - 16): the transposed flags
      const int r = t - 16;
      if (!diag && j0 + r < G) {
        unsigned w = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) w |= (sflag[c * 17 + r] != 0.0f ? 1u : 0u) << c;
        bits[(size_t)(j0 + r) * (pitch >> 1) + ti] = (uint16_t)w;
      }
    } else if (diag && t < 96) {                    // the pad pieces of the rows i0 .. i0 + 15 (at most three per row)
      const int r = (t - 32) & 15, w = T + ((t - 32) >> 4);
      if (i0 + r < G && w < (pitch >> 1)) bits[(size_t)(i0 + r) * (pitch >> 1) + w] = 0;
    }
  }
}

// Greedy leader prune over the threshold bit-matrix, in conformer order: ONE wave.  Lane l holds columns 64 l .. 64 l + 63 of
// the kept set and of every row as one 64-bit word.  The address of row i does not depend on what became of row i - 1, so
// AG_PRUNE_DEPTH rows are loaded ahead of the sequential walk.  leader / count are staged in LDS and written once, coalesced.
#define AG_PRUNE_DEPTH 16
__global__ void __launch_bounds__(64) k_leader_prune(const uint64_t* __restrict__ bits, int G, int words, int32_t* __restrict__ keep,
                                                     int32_t* __restrict__ leader, int32_t* __restrict__ count,
                                                     int32_t* __restrict__ n_kept) {
  __shared__ int32_t s_leader[AGDIFF_PRUNE_MAX_CONFS];
  __shared__ int32_t s_count[AGDIFF_PRUNE_MAX_CONFS];
  const int lane = threadIdx.x;
  uint64_t kept = 0;
  uint64_t cur[AG_PRUNE_DEPTH], nxt[AG_PRUNE_DEPTH];
#pragma unroll
  for (int d = 0; d < AG_PRUNE_DEPTH; ++d) cur[d] = (d < G && lane < words) ? bits[(size_t)d * words + lane] : 0;
  for (int base = 0; base < G; base += AG_PRUNE_DEPTH) {
#pragma unroll
    for (int d = 0; d < AG_PRUNE_DEPTH; ++d) {
      const int r = base + AG_PRUNE_DEPTH + d;
      nxt[d] = (r < G && lane < words) ? bits[(size_t)r * words + lane] : 0;
    }
#pragma unroll
    for (int d = 0; d < AG_PRUNE_DEPTH; ++d) {
      const int i = base + d;
      if (i < G) {                                  // (wave-uniform)
        const uint64_t hit = cur[d] & kept;         // kept holds only j < i
        const unsigned long long any = __ballot(hit != 0);
        if (any == 0) {
          if (lane == (i >> 6)) kept |= 1ull << (i & 63);
          if (lane == 0) { s_leader[i] = i; s_count[i] = 1; }
        } else {
          const int first = __ffsll((long long)any) - 1;
          if (lane == first) {
            const int l = first * 64 + __ffsll((long long)hit) - 1;      // the smallest kept j with bit (i, j)
            s_leader[i] = l;
            s_count[l] += 1;
            s_count[i] = 0;
          }
        }
      }
    }
#pragma unroll
    for (int d = 0; d < AG_PRUNE_DEPTH; ++d) cur[d] = nxt[d];
  }
  __syncthreads();
  for (int i = lane; i < G; i += 64) {
    const int l = s_leader[i];
    leader[i] = l;
    keep[i] = l == i ? 1 : 0;
    count[i] = s_count[i];
  }
  int k = __popcll(kept);
  ag_wave_sum(k);
  if (lane == 0) n_kept[0] = k;
}

// Taylor-Butina clustering over the threshold bit-matrix (the rule: include/agdiff_hip.h, agdiff_butina_cluster): ONE workgroup
// of AG_BUTINA_THREADS / 64 waves.  In LDS: the neighbour count of every conformer (s_cnt, one pad slot per 64 so that the lanes
// that own columns 64 l + b of a row spread over the banks), the live set and the current cluster as 64 words each, and per
// conformer its centroid, per centroid its cluster's size and rank, as 16-bit values (all < 65536) -- 42 KB.
// Every iteration: a block-wide arg-max over the packed keys count << 12 | (4095 - index) of the live conformers (a count reaches
// 4096: 13 bits), then wave 0 ANDs the centroid's row with the live set.  reorder = 1: the counts follow the live set through the
// REMOVED members' rows -- each still-live j with bit (m, j) loses one, by LDS atomics -- so every row is read once over the whole
// run.  Once the best count is 1 (in either mode) nobody live has a neighbour left to take, so the rest are singletons in index
// order and are finished in one pass.  The outer loop is counted and its centroid always leaves the live set; every barrier in it sits under a
// condition read from LDS after a barrier, the same in every thread.
#define AG_BUTINA_THREADS 1024
#define AG_BUTINA_WAVES (AG_BUTINA_THREADS / 64)
#define AG_BUTINA_DEPTH 4                           // rows a wave keeps in flight
__device__ __forceinline__ int ag_butina_slot(int i) { return i + (i >> 6); }

__global__ void __launch_bounds__(AG_BUTINA_THREADS) k_butina_cluster(const uint64_t* __restrict__ bits, int G, int words, int reorder,
                                                                      int32_t* __restrict__ leader, int32_t* __restrict__ count,
                                                                      int32_t* __restrict__ rank, int32_t* __restrict__ n_clusters) {
  __shared__ int32_t s_cnt[AGDIFF_PRUNE_MAX_CONFS + 64];
  __shared__ uint16_t s_leader[AGDIFF_PRUNE_MAX_CONFS];
  __shared__ uint16_t s_size[AGDIFF_PRUNE_MAX_CONFS];
  __shared__ uint16_t s_rank[AGDIFF_PRUNE_MAX_CONFS];
  __shared__ uint64_t s_live[64];
  __shared__ uint64_t s_mem[64];
  __shared__ int32_t s_best[AG_BUTINA_WAVES];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t < 64) s_live[t] = G >= 64 * t + 64 ? ~0ull : (G > 64 * t ? (1ull << (G - 64 * t)) - 1 : 0);   // columns >= G never count
  __syncthreads();
  {                                                 // the counts over all G conformers: one wave per row, diagonal taken as set
    const uint64_t all = s_live[lane];
    for (int base = wv * AG_BUTINA_DEPTH; base < G; base += AG_BUTINA_WAVES * AG_BUTINA_DEPTH) {
      uint64_t w[AG_BUTINA_DEPTH];
#pragma unroll
      for (int d = 0; d < AG_BUTINA_DEPTH; ++d) w[d] = (base + d < G && lane < words) ? bits[(size_t)(base + d) * words + lane] : 0;
#pragma unroll
      for (int d = 0; d < AG_BUTINA_DEPTH; ++d) {
        const int r = base + d;
        if (r < G) {                                // (wave-uniform)
          const uint64_t x = w[d] | (lane == (r >> 6) ? 1ull << (r & 63) : 0);
          int p = __popcll(x & all);
          ag_wave_sum(p);
          if (lane == 0) s_cnt[ag_butina_slot(r)] = p;
        }
      }
    }
  }
  __syncthreads();
  int nclus = 0;
  for (int it = 0; it < G; ++it) {
    int key = -1;                                   // (a dead conformer; a live one has key >= 0)
    for (int i = t; i < G; i += AG_BUTINA_THREADS) {
      const int c = s_cnt[ag_butina_slot(i)];
      const int k = ((c > 0 ? c : 0) << 12) | (AGDIFF_PRUNE_MAX_CONFS - 1 - i);
      key = max(key, ((s_live[i >> 6] >> (i & 63)) & 1) ? k : -1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o));
    if (lane == 0) s_best[wv] = key;
    __syncthreads();
    int best = s_best[0];
#pragma unroll
    for (int w = 1; w < AG_BUTINA_WAVES; ++w) best = max(best, s_best[w]);
    if (best < 0) break;                            // nobody is live
    const int c = AGDIFF_PRUNE_MAX_CONFS - 1 - (best & (AGDIFF_PRUNE_MAX_CONFS - 1));
    if ((best >> 12) <= 1) {                        // only singletons are left: index order
      const int pc = __popcll(s_live[lane]);        // every wave: the live conformers below each word, by a prefix sum over the lanes
      int upto = pc;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(upto, o);
        upto += lane >= o ? v : 0;
      }
      const int total = __shfl(upto, 63);
      for (int base = 64 * wv; base < G; base += AG_BUTINA_THREADS) {      // (wave-uniform: word base / 64, conformer base + lane)
        const int before = __shfl(upto - pc, base >> 6);
        const uint64_t lw = s_live[base >> 6];
        const int i = base + lane;
        if ((lw >> lane) & 1) {                     // (live bits lie below G)
          s_leader[i] = (uint16_t)i;
          s_size[i] = 1;
          s_rank[i] = (uint16_t)(nclus + before + __popcll(lw & ((1ull << lane) - 1)));
        }
      }
      nclus += total;
      break;
    }
    if (wv == 0) {                                  // the cluster of c: c and its live neighbours
      const uint64_t w = (lane < words ? bits[(size_t)c * words + lane] : 0) | (lane == (c >> 6) ? 1ull << (c & 63) : 0);
      const uint64_t mem = w & s_live[lane];
      s_mem[lane] = mem;
      s_live[lane] &= ~mem;
      for (uint64_t m = mem; m; m &= m - 1) s_leader[64 * lane + __ffsll((long long)m) - 1] = (uint16_t)c;
      int p = __popcll(mem);
      ag_wave_sum(p);
      if (lane == 0) { s_size[c] = (uint16_t)p; s_rank[c] = (uint16_t)it; }
    }
    nclus = it + 1;
    __syncthreads();
    if (reorder) {                                  // (block-uniform) the removed members' rows take them out of the live counts
      const uint64_t live = s_live[lane];
      for (int l = wv; l < words; l += AG_BUTINA_WAVES) {
        uint64_t m = s_mem[l];                      // (wave-uniform)
        while (m) {
          int r[AG_BUTINA_DEPTH];
          uint64_t w[AG_BUTINA_DEPTH];
#pragma unroll
          for (int d = 0; d < AG_BUTINA_DEPTH; ++d) {
            r[d] = m ? 64 * l + __ffsll((long long)m) - 1 : -1;
            m &= m - 1;
          }
#pragma unroll
          for (int d = 0; d < AG_BUTINA_DEPTH; ++d) w[d] = (r[d] >= 0 && lane < words) ? bits[(size_t)r[d] * words + lane] : 0;
#pragma unroll
          for (int d = 0; d < AG_BUTINA_DEPTH; ++d)
            for (uint64_t x = w[d] & live; x; x &= x - 1) atomicSub(&s_cnt[ag_butina_slot(64 * lane + __ffsll((long long)x) - 1)], 1);
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int i = t; i < G; i += AG_BUTINA_THREADS) {
    const int l = s_leader[i];
    leader[i] = l;
    count[i] = l == i ? (int)s_size[i] : 0;
    rank[i] = s_rank[l];
  }
  if (t == 0) n_clusters[0] = nclus;
}

// MaxMin picking over the float matrix (the rule: include/agdiff_hip.h, agdiff_maxmin_pick): ONE workgroup of AG_MAXMIN_THREADS / 64
// waves.  Thread t owns the columns t, t + 1024, ... (AG_MAXMIN_COLS of them at the limit) and keeps their near, owner and state
// in registers; a column >= G is ineligible from the start and is never read or written.  Every iteration: the last pick's row is
// read with one coalesced 4-byte load per owned column (no alignment beyond the element's, any G), the min-update, then a
// block-wide arg-max over the 64-bit keys  bits(near) << 32 | ~index  of the eligible unpicked columns -- near is a finite
// non-negative fp32 there with -0 taken as +0, so its bit pattern orders as the value does, and the complement of the index
// sends ties to the lowest; 0 is no candidate (a real key has a low half >= ~4095).  The arg-max is a wave reduction by shuffles,
// 16 partials through LDS and a second reduction that every wave does for itself; the partials are double-buffered, so an
// iteration costs ONE barrier: the buffer written in iteration r + 1 was last read before the barrier of iteration r.  The
// outer loop is counted (at most K iterations, one dependent row read each) and every thread leaves it on the same value read
// from LDS after the barrier.
#define AG_MAXMIN_THREADS 1024
#define AG_MAXMIN_WAVES (AG_MAXMIN_THREADS / 64)
#define AG_MAXMIN_COLS (AGDIFF_PRUNE_MAX_CONFS / AG_MAXMIN_THREADS)
static_assert(AG_MAXMIN_COLS * AG_MAXMIN_THREADS == AGDIFF_PRUNE_MAX_CONFS && AG_MAXMIN_WAVES == 16, "k_maxmin_pick: 4096 columns, 16 waves");

__device__ __forceinline__ uint64_t ag_max_u64_xor(uint64_t k, int o) {
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), o), lo = (uint32_t)__shfl_xor((int)(uint32_t)k, o);
  const uint64_t other = ((uint64_t)hi << 32) | lo;
  return other > k ? other : k;
}

__global__ void __launch_bounds__(AG_MAXMIN_THREADS) k_maxmin_pick(const float* __restrict__ dist, int G, int K, int first, float stop,
                                                                   int32_t* __restrict__ picks, float* __restrict__ radius,
                                                                   int32_t* __restrict__ owner, float* __restrict__ near,
                                                                   int32_t* __restrict__ n_picked, float* __restrict__ cover) {
  enum { OPEN = 0, PICKED = 1, OUT = 2 };           // eligible and unpicked / a pick / ineligible for good (or a column >= G)
  __shared__ uint64_t s_part[2][AG_MAXMIN_WAVES];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  float nr[AG_MAXMIN_COLS];
  int ow[AG_MAXMIN_COLS], state[AG_MAXMIN_COLS];
#pragma unroll
  for (int c = 0; c < AG_MAXMIN_COLS; ++c) {
    const int j = t + c * AG_MAXMIN_THREADS;
    nr[c] = j == first ? 0.0f : __builtin_inff();
    ow[c] = j == first ? 0 : -1;
    state[c] = j >= G ? OUT : (j == first ? PICKED : OPEN);
  }
  if (t == 0) { picks[0] = first; radius[0] = __builtin_inff(); }
  int n = 1, last = first;
  float cov = 0.0f;
  for (int r = 0; r < K; ++r) {                     // pick r's row; n == r + 1 here
    const float* __restrict__ row = dist + (size_t)last * (size_t)G;
    float v[AG_MAXMIN_COLS];
#pragma unroll
    for (int c = 0; c < AG_MAXMIN_COLS; ++c) {
      const int j = t + c * AG_MAXMIN_THREADS;
      v[c] = (j < G && state[c] == OPEN) ? row[j] : 0.0f;
    }
    uint64_t key = 0;
#pragma unroll
    for (int c = 0; c < AG_MAXMIN_COLS; ++c) {
      const int j = t + c * AG_MAXMIN_THREADS;
      if (state[c] == OPEN) {
        const float x = v[c] == 0.0f ? 0.0f : v[c];                  // (-0 is +0)
        if (!(x >= 0.0f) || x == __builtin_inff()) {
          state[c] = OUT;
        } else {
          if (x < nr[c]) { nr[c] = x; ow[c] = r; }
          const uint64_t k = ((uint64_t)__float_as_uint(nr[c]) << 32) | (uint32_t)~(uint32_t)j;
          key = k > key ? k : key;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = ag_max_u64_xor(key, o);
    if (lane == 0) s_part[r & 1][wv] = key;
    __syncthreads();
    uint64_t best = s_part[r & 1][lane & (AG_MAXMIN_WAVES - 1)];
#pragma unroll
    for (int o = AG_MAXMIN_WAVES / 2; o > 0; o >>= 1) best = ag_max_u64_xor(best, o);
    if (best == 0) break;                           // no candidate is left: cover = 0
    const int cand = (int)~(uint32_t)best;
    const float far = __uint_as_float((uint32_t)(best >> 32));
    if (!(n < K && far > stop)) {                   // the candidate is not picked: the walk ends
      cov = far;
      break;
    }
#pragma unroll
    for (int c = 0; c < AG_MAXMIN_COLS; ++c)
      if (t + c * AG_MAXMIN_THREADS == cand) { state[c] = PICKED; nr[c] = 0.0f; ow[c] = n; }
    if (t == 0) { picks[n] = cand; radius[n] = far; }
    last = cand;
    ++n;
  }
#pragma unroll
  for (int c = 0; c < AG_MAXMIN_COLS; ++c) {
    const int j = t + c * AG_MAXMIN_THREADS;
    if (j < G) {
      owner[j] = state[c] == OUT ? -1 : ow[c];
      near[j] = state[c] == OUT ? __builtin_nanf("") : nr[c];
    }
  }
  for (int i = n + t; i < K; i += AG_MAXMIN_THREADS) {
    picks[i] = -1;
    radius[i] = __builtin_nanf("");
  }
  if (t == 0) { n_picked[0] = n; cover[0] = cov; }
}

// Alternating k-medoids over the float matrix (the rule: include/agdiff_hip.h, agdiff_kmedoids).  Unlike the two walks above an
// iteration is parallel inside, so it is a SEQUENCE OF LAUNCHES, and the kernel boundary is the only grid-wide ordering there is:
//   k_kmed_init     one workgroup: checks the seeds (range, duplicates by LDS counters, eligibility), sets up the control words;
//                   on a bad seed it writes the status-2 fill and sets `done`, so nothing after it does anything
//   k_kmed_assign   the column pass (ag_kmed_columns<false>, below) under the anchor init[0]: writes labels and near
//   k_kmed_costs    one wave per candidate row i: sum of Q(dist[i][j]) over the members j != i of i's cluster, uint64 partials
//                   reduced by shuffles; writes the key cost << 12 | i (all ones for an ineligible row)
//   k_kmed_choose   one workgroup (G keys, nothing to stream): per-cluster arg-min by LDS atomic min on the keys, the incumbent
//                   rule, the changed flag; counts the update and sets status / done
//   k_kmed_finish   one workgroup: size, within (uint64 LDS sums of Q(near)), cost, n_iter, status
// The state between launches lives in the outputs (medoids, labels, near) and in `work`: 8 control words, then the G keys.
// Every kernel of the loop reads ctl[KM_DONE] first and returns when it is set.  Sums and comparisons are on integers, LDS
// atomics are min / add on integers, there are no global atomics and no workgroup waits on another: nothing depends on the
// order in which workgroups run.  Every loop is counted.
#define AG_KMED_MAX_DIST 4096.0f
enum { KM_DONE = 0, KM_STATUS = 1, KM_ITERS = 2, KM_CTL_WORDS = 8 };     // int32 words at the head of `work`
static_assert(AGDIFF_KMEDOIDS_WORK_BYTES >= KM_CTL_WORDS * 4 + AGDIFF_PRUNE_MAX_CONFS * 8, "agdiff_kmedoids: control words + one key per conformer");
static_assert(AGDIFF_PRUNE_MAX_CONFS == 1 << 12 && AGDIFF_KMEDOIDS_MAX_DIST == 4096, "agdiff_kmedoids: 12 index bits under a sum of 4096 terms <= 2^40");

__device__ __forceinline__ bool ag_kmed_valid(float x) { return x >= 0.0f && x <= AG_KMED_MAX_DIST; }

// Q(x): rint(x * 2^28) for a valid x, 2^40 otherwise.  x * 2^28 < 2^41 is exact in fp64, and adding 2^52 rounds it to an
// integer, half to even, in the one rounding of the fma; the integer is then the low 52 bits.
__device__ __forceinline__ uint64_t ag_kmed_q(float x) {
  const double s = __builtin_fma((double)x, 268435456.0, 4503599627370496.0);
  const uint64_t q = (uint64_t)__double_as_longlong(s) & ((1ull << 52) - 1);
  return ag_kmed_valid(x) ? q : (1ull << 40);
}

// the status-2 fill of agdiff_kmedoids, agdiff_pam_build and agdiff_pam_swap, by one workgroup of 1024 threads: every output is
// written and `done` is set, so nothing after it does anything
__device__ __forceinline__ void ag_kmed_fill_bad(int G, int K, int32_t* __restrict__ medoids, int32_t* __restrict__ labels,
                                                 float* __restrict__ near, int32_t* __restrict__ size, double* __restrict__ within,
                                                 double* __restrict__ cost, int32_t* __restrict__ n_iter, int32_t* __restrict__ status,
                                                 int32_t* __restrict__ ctl) {
  const int t = threadIdx.x;
  for (int r = t; r < K; r += 1024) { medoids[r] = -1; size[r] = 0; within[r] = 0.0; }
  for (int j = t; j < G; j += 1024) { labels[j] = -1; near[j] = __builtin_nanf(""); }
  if (t < KM_CTL_WORDS) ctl[t] = t == KM_DONE ? 1 : (t == KM_STATUS ? 2 : 0);
  if (t == 0) { cost[0] = 0.0; n_iter[0] = 0; status[0] = 2; }
}

// the seed check of agdiff_kmedoids (s0 = init[0], status0 = 0) and of agdiff_pam_swap (s0 = its anchor, status0 = 1: "a negative
// exchange may be left" until a choose says otherwise), by one workgroup of 1024 threads: s0's row decides who is eligible
__device__ __forceinline__ void ag_kmed_check_seeds(const float* __restrict__ dist, int G, int K, const int32_t* __restrict__ init, int s0,
                                                    int status0, int32_t* __restrict__ medoids, int32_t* __restrict__ labels,
                                                    float* __restrict__ near, int32_t* __restrict__ size, double* __restrict__ within,
                                                    double* __restrict__ cost, int32_t* __restrict__ n_iter, int32_t* __restrict__ status,
                                                    int32_t* __restrict__ ctl) {
  __shared__ int32_t s_seen[AGDIFF_PRUNE_MAX_CONFS];
  const int t = threadIdx.x;
  for (int j = t; j < G; j += 1024) s_seen[j] = 0;
  __syncthreads();
  const bool s0_ok = (unsigned)s0 < (unsigned)G;    // (block-uniform)
  int bad = s0_ok ? 0 : 1;
  if (s0_ok) {
    for (int r = t; r < K; r += 1024) {
      const int s = init[r];
      if ((unsigned)s >= (unsigned)G) { bad = 1; continue; }
      if (atomicAdd(&s_seen[s], 1) != 0) bad = 1;                           // a duplicate: somebody counted this seed before
      if (s != s0 && !ag_kmed_valid(dist[(size_t)s0 * (size_t)G + s])) bad = 1;   // an ineligible seed
    }
  }
  bad = __syncthreads_or(bad);
  if (!bad) {
    for (int r = t; r < K; r += 1024) medoids[r] = init[r];
    if (t < KM_CTL_WORDS) ctl[t] = t == KM_STATUS ? status0 : 0;
    return;
  }
  ag_kmed_fill_bad(G, K, medoids, labels, near, size, within, cost, n_iter, status, ctl);
}

__global__ void __launch_bounds__(1024) k_kmed_init(const float* __restrict__ dist, int G, int K, const int32_t* __restrict__ init,
                                                    int32_t* __restrict__ medoids, int32_t* __restrict__ labels, float* __restrict__ near,
                                                    int32_t* __restrict__ size, double* __restrict__ within, double* __restrict__ cost,
                                                    int32_t* __restrict__ n_iter, int32_t* __restrict__ status, int32_t* __restrict__ ctl) {
  ag_kmed_check_seeds(dist, G, K, init, init[0], 0, medoids, labels, near, size, within, cost, n_iter, status, ctl);
}

// k joins the running (best key, second-best Q + 1) of one column; ~0 is "none" in both places.  Keys differ in their rank bits.
__device__ __forceinline__ void ag_kmed_push(uint64_t& k1, uint64_t& s2, uint64_t k) {
  const bool lower = k < k1;
  const uint64_t loser = lower ? k1 : k;
  k1 = lower ? k : k1;
  const uint64_t ls = loser == ~0ull ? ~0ull : loser >> 12;
  s2 = ls < s2 ? ls : s2;
}

// THE COLUMN PASS, the body of k_kmed_assign (SECOND = false) and k_pam_state (SECOND = true), by a workgroup of 256 threads: 64
// columns, its 4 waves take the ranks r = w, w + 4, ... of the K medoid rows (coalesced 4-byte loads, unrolled); the keys
// (Q + 1) << 12 | r -- 0 << 12 | r for the medoid's own column -- are min-reduced through LDS: lowest Q, then lowest rank.  Row
// `anchor` decides who is eligible.  Writes labels and near; with SECOND the second-best Q + 1 is kept beside the best key, and
// dn, ds (all ones: none) and tag = -1 (ineligible) or n << 1 | is-a-medoid are written too.  Without it `sec` is never stored,
// so nothing of it is left in the code.
template <bool SECOND>
__device__ __forceinline__ void ag_kmed_columns(const float* __restrict__ dist, int G, int K, int anchor,
                                                const int32_t* __restrict__ medoids, int32_t* __restrict__ labels,
                                                float* __restrict__ near, uint64_t* __restrict__ dn, uint64_t* __restrict__ ds,
                                                int32_t* __restrict__ tag) {
  __shared__ uint64_t s_key[SECOND ? 2 : 1][4][64];     // the best keys, then the seconds
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const bool in = j < G;
  const int jc = in ? j : G - 1;                    // (a column past the end reads the last one and writes nothing)
  uint64_t key = ~0ull, sec = ~0ull;
#pragma unroll 4
  for (int r = wv; r < K; r += 4) {
    const int m = medoids[r];                       // (wave-uniform)
    const float x = dist[(size_t)m * (size_t)G + jc];
    ag_kmed_push(key, sec, (m == jc ? 0ull : (ag_kmed_q(x) + 1) << 12) | (uint64_t)r);
  }
  s_key[0][wv][lane] = key;
  if (SECOND) s_key[1][wv][lane] = sec;
  __syncthreads();
  if (wv != 0 || !in) return;
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    ag_kmed_push(key, sec, s_key[0][w][lane]);
    if (SECOND) {
      const uint64_t s = s_key[1][w][lane];
      sec = s < sec ? s : sec;
    }
  }
  const bool eligible = j == anchor || ag_kmed_valid(dist[(size_t)anchor * (size_t)G + j]);
  const int r = (int)(key & 4095);
  const int m = medoids[r];
  const float x = dist[(size_t)m * (size_t)G + j];
  labels[j] = eligible ? r : -1;
  near[j] = !eligible ? __builtin_nanf("") : ((key >> 12) == 0 || x == 0.0f ? 0.0f : x);     // (-0 is written as +0)
  if (SECOND) {
    tag[j] = eligible ? (r << 1) | (m == j ? 1 : 0) : -1;
    dn[j] = (key >> 12) == 0 ? 0ull : (key >> 12) - 1;
    ds[j] = sec == ~0ull ? ~0ull : sec - 1;         // (K == 1: no other rank, min(ds, x) = x)
  }
}

// final = 0: an assign of the loop, skipped once `done` is set.  final = 1: the assign after the last update, which runs only
// after a status-1 stop (after a status-0 stop the labels already belong to the returned medoids).
__global__ void __launch_bounds__(256) k_kmed_assign(const float* __restrict__ dist, int G, int K, const int32_t* __restrict__ init,
                                                     const int32_t* __restrict__ medoids, int32_t* __restrict__ labels,
                                                     float* __restrict__ near, const int32_t* __restrict__ ctl, int final) {
  if (final ? ctl[KM_STATUS] != 1 : ctl[KM_DONE] != 0) return;
  ag_kmed_columns<false>(dist, G, K, init[0], medoids, labels, near, nullptr, nullptr, nullptr);
}

__global__ void __launch_bounds__(256) k_kmed_costs(const float* __restrict__ dist, int G, const int32_t* __restrict__ labels,
                                                    uint64_t* __restrict__ keys, const int32_t* __restrict__ ctl) {
  if (ctl[KM_DONE] != 0) return;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);     // (wave-uniform)
  if (i >= G) return;
  const int c = labels[i];
  if (c < 0) {
    if (lane == 0) keys[i] = ~0ull;
    return;
  }
  const float* __restrict__ row = dist + (size_t)i * (size_t)G;
  uint64_t sum = 0;
#pragma unroll 8
  for (int j = lane; j < G; j += 64) {
    const float x = row[j];
    const int l = labels[j];
    sum += (l == c && j != i) ? ag_kmed_q(x) : 0ull;
  }
  ag_wave_sum(sum);
  if (lane == 0) keys[i] = (sum << 12) | (uint64_t)i;
}

// the per-cluster arg-min of k_kmed_choose and k_link_medoids, by one workgroup of 1024 threads: s_best[r] becomes the smallest
// key cost << 12 | index among the members of rank r (all ones: no member) -- lowest cost, then lowest index.  Ends on a barrier.
__device__ __forceinline__ void ag_kmed_best(int G, int K, const int32_t* __restrict__ labels, const uint64_t* __restrict__ keys,
                                             unsigned long long* s_best) {
  const int t = threadIdx.x;
  for (int r = t; r < K; r += 1024) s_best[r] = ~0ull;
  __syncthreads();
  for (int j = t; j < G; j += 1024) {
    const int l = labels[j];
    if (l >= 0) atomicMin(&s_best[l], (unsigned long long)keys[j]);   // lowest cost, then lowest index
  }
  __syncthreads();
}

__global__ void __launch_bounds__(1024) k_kmed_choose(int G, int K, int max_iter, const int32_t* __restrict__ labels,
                                                      const uint64_t* __restrict__ keys, int32_t* __restrict__ medoids,
                                                      int32_t* __restrict__ ctl) {
  if (ctl[KM_DONE] != 0) return;                    // (block-uniform: ctl is written only after the barriers below)
  __shared__ unsigned long long s_best[AGDIFF_PRUNE_MAX_CONFS];
  const int t = threadIdx.x;
  ag_kmed_best(G, K, labels, keys, s_best);
  int changed = 0;
  for (int r = t; r < K; r += 1024) {
    const uint64_t best = s_best[r], mine = keys[medoids[r]];
    if ((best >> 12) != (mine >> 12)) {             // the incumbent stays when its cost equals the minimum
      medoids[r] = (int)(best & 4095);
      changed = 1;
    }
  }
  changed = __syncthreads_or(changed);
  if (t == 0) {
    const int n = ctl[KM_ITERS] + 1;
    ctl[KM_ITERS] = n;
    if (!changed) { ctl[KM_STATUS] = 0; ctl[KM_DONE] = 1; }
    else if (n >= max_iter) { ctl[KM_STATUS] = 1; ctl[KM_DONE] = 1; }
  }
}

__global__ void __launch_bounds__(1024) k_kmed_finish(int G, int K, const int32_t* __restrict__ labels, const float* __restrict__ near,
                                                      int32_t* __restrict__ size, double* __restrict__ within, double* __restrict__ cost,
                                                      int32_t* __restrict__ n_iter, int32_t* __restrict__ status,
                                                      const int32_t* __restrict__ ctl) {
  if (ctl[KM_STATUS] == 2) return;                  // a bad seed: k_kmed_init wrote everything
  __shared__ unsigned long long s_sum[AGDIFF_PRUNE_MAX_CONFS];
  __shared__ int32_t s_size[AGDIFF_PRUNE_MAX_CONFS];
  __shared__ unsigned long long s_part[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (int r = t; r < K; r += 1024) { s_sum[r] = 0; s_size[r] = 0; }
  __syncthreads();
  uint64_t total = 0;
  for (int j = t; j < G; j += 1024) {
    const int l = labels[j];
    if (l >= 0) {
      const uint64_t q = ag_kmed_q(near[j]);
      atomicAdd(&s_sum[l], (unsigned long long)q);
      atomicAdd(&s_size[l], 1);
      total += q;
    }
  }
  ag_wave_sum(total);
  if (lane == 0) s_part[wv] = total;
  __syncthreads();
  for (int r = t; r < K; r += 1024) {
    size[r] = s_size[r];
    within[r] = (double)s_sum[r] * (1.0 / 268435456.0);              // (<= 2^52: exact)
  }
  if (t == 0) {
    uint64_t all = 0;
    for (int w = 0; w < 16; ++w) all += s_part[w];
    cost[0] = (double)all * (1.0 / 268435456.0);
    n_iter[0] = ctl[KM_ITERS];
    status[0] = ctl[KM_STATUS];
  }
}

// THE ROW PASS, the scaffold of k_sil_rows and k_pam_rows, by a workgroup of 256 threads: row i of the matrix is streamed once with
// coalesced 4-byte loads and integer terms of its entries are added into K uint64 bins in LDS, one per rank (LDS 64-bit integer
// add, as k_kmed_finish); then the row's threads stride over the bins and min-reduce (value, rank) pairs under the total order
// "lowest value, then lowest rank".  What is added and what the pairs hold is the kernel's own; who shares a row, where its bins
// are, their zeroing and the reduction are here.  Two shapes, chosen by K (ag_row_pass_launch, below) so that the bins of a
// workgroup take at most 32 KB of LDS (AG_ROW_BIN_BYTES):
//   K <= AG_ROW_WAVE_MAX_K (1024)   ROWS = 4: one row per WAVE, four rows and 4 K bins per workgroup
//   K >  AG_ROW_WAVE_MAX_K          ROWS = 1: one row per WORKGROUP of four waves, K bins (K <= 4096)
#define AG_ROW_WAVE_MAX_K 1024
enum { AG_ROW_BIN_BYTES = 32768 };                // the most LDS a workgroup's bins take, in either shape
static_assert(4 * AG_ROW_WAVE_MAX_K * 8 <= AG_ROW_BIN_BYTES && AGDIFF_PRUNE_MAX_CONFS * 8 <= AG_ROW_BIN_BYTES, "the row pass: the bins of either shape fit their LDS");

// the smaller of two (value, index) pairs: lowest value, then lowest index.  The values are never NaN.
template <typename V>
__device__ __forceinline__ void ag_min_pair(V& v, int& c, V ov, int oc) {
  const bool take = ov < v || (ov == v && oc < c);
  v = take ? ov : v;
  c = take ? oc : c;
}

// the smallest pair of the WAVES waves of the workgroup, in every thread: a wave xor-butterfly, then (WAVES > 1) the waves'
// partials through LDS, which every wave of the workgroup has to reach.  The slots are the helper's own and nothing orders
// their reads before a later write: one call per instantiation and kernel, or a barrier between two.
template <int WAVES, typename V>
__device__ __forceinline__ void ag_min_pair_over(V& v, int& c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ag_min_pair(v, c, __shfl_xor(v, o), __shfl_xor(c, o));
  if constexpr (WAVES > 1) {
    __shared__ V s_v[WAVES];
    __shared__ int s_c[WAVES];
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = v; s_c[threadIdx.x >> 6] = c; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; ++w) ag_min_pair(v, c, s_v[w], s_c[w]);
  }
}

template <int ROWS>
struct ag_row_pass {
  static_assert(ROWS == 1 || ROWS == 4, "one row per workgroup or one per wave");
  static constexpr int NT = ROWS == 4 ? 64 : 256;   // the threads that share a row
  int tid;                                          // this thread among them
  int i;                                            // the row (wave-uniform; may be >= G: every wave reaches every barrier)
  unsigned long long* bins;                         // the row's K bins, of s_bins [ROWS][K]
  __device__ __forceinline__ ag_row_pass(unsigned long long* s_bins, int K) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    tid = ROWS == 4 ? lane : (int)threadIdx.x;
    i = ROWS == 4 ? blockIdx.x * 4 + wv : (int)blockIdx.x;
    bins = s_bins + (ROWS == 4 ? (size_t)wv * (size_t)K : 0);
  }
  __device__ __forceinline__ void zero_bins(int K) const {
    for (int c = tid; c < K; c += NT) bins[c] = 0ull;
    __syncthreads();
  }
  template <typename V>
  __device__ __forceinline__ void min_pair(V& v, int& c) const { ag_min_pair_over<ROWS == 4 ? 1 : 4>(v, c); }
};

// Silhouette coefficients of a given clustering over the same float matrix (the rule: include/agdiff_hip.h, agdiff_silhouette).
// Three launches, the kernel boundary again the only grid-wide ordering:
//   k_sil_init     one workgroup: checks the labels (-1 or a rank in [0, K)), counts the members of every rank with LDS integer
//                  atomics and writes `size` and the control words; on a bad label it writes the status-2 fill and sets `done`
//   k_sil_rows     the row pass: Q of row i's entries goes into the bin of the entry's rank; the pairs are (m_c, c), the means
//                  m_c = S_c / size[c]; one lane writes a, b, s, other and T(i) = rint(s 2^40) into `work`
//   k_sil_finish   one workgroup: per-rank and total sums of T (int64, as uint64 LDS adds), the divisions, status
// The state between launches lives in `size` and in `work`: the 8 control words (KM_DONE, KM_STATUS), then T [G].  Sums are on
// integers; the only floating-point values that cross lanes are the means of the (mean, rank) pairs, compared and never added;
// LDS atomics are adds on integers, there are no global atomics and no workgroup waits on another.  Every loop is counted.
static_assert(AGDIFF_SILHOUETTE_WORK_BYTES >= KM_CTL_WORDS * 4 + AGDIFF_PRUNE_MAX_CONFS * 8, "agdiff_silhouette: control words + one T per conformer");
static_assert(AGDIFF_PRUNE_MAX_CONFS == 1 << 12 && AGDIFF_KMEDOIDS_MAX_DIST == 4096, "agdiff_silhouette: a row's sum of 4096 terms <= 2^40 and a sum of 4096 |T| <= 2^40 stay <= 2^52");

__global__ void __launch_bounds__(1024) k_sil_init(int G, int K, const int32_t* __restrict__ labels, double* __restrict__ a,
                                                   double* __restrict__ b, double* __restrict__ s, int32_t* __restrict__ other,
                                                   int32_t* __restrict__ size, double* __restrict__ cluster_mean,
                                                   double* __restrict__ mean, int32_t* __restrict__ status, int32_t* __restrict__ ctl) {
  __shared__ int32_t s_size[AGDIFF_PRUNE_MAX_CONFS];
  const int t = threadIdx.x;
  for (int r = t; r < K; r += 1024) s_size[r] = 0;
  __syncthreads();
  int bad = 0;
  for (int j = t; j < G; j += 1024) {
    const int l = labels[j];
    if (l == -1) continue;
    if ((unsigned)l >= (unsigned)K) { bad = 1; continue; }
    atomicAdd(&s_size[l], 1);
  }
  bad = __syncthreads_or(bad);
  if (!bad) {
    for (int r = t; r < K; r += 1024) size[r] = s_size[r];
    if (t < KM_CTL_WORDS) ctl[t] = 0;
    return;
  }
  const double nan = __builtin_nan("");
  for (int j = t; j < G; j += 1024) { a[j] = nan; b[j] = nan; s[j] = nan; other[j] = -1; }
  for (int r = t; r < K; r += 1024) { size[r] = 0; cluster_mean[r] = nan; }
  if (t < KM_CTL_WORDS) ctl[t] = t == KM_DONE ? 1 : (t == KM_STATUS ? 2 : 0);
  if (t == 0) { mean[0] = nan; status[0] = 2; }
}

// the pairs are (mean, rank); "none" is (+inf, INT_MAX)
template <int ROWS>
__global__ void __launch_bounds__(256) k_sil_rows(const float* __restrict__ dist, int G, int K, const int32_t* __restrict__ labels,
                                                  const int32_t* __restrict__ size, double* __restrict__ a, double* __restrict__ b,
                                                  double* __restrict__ s, int32_t* __restrict__ other, int64_t* __restrict__ T,
                                                  const int32_t* __restrict__ ctl) {
  if (ctl[KM_DONE] != 0) return;                    // (grid-uniform: a bad label, k_sil_init wrote everything)
  extern __shared__ unsigned long long s_bins[];    // [ROWS][K]
  const ag_row_pass<ROWS> rp(s_bins, K);
  const int NT = rp.NT, tid = rp.tid, i = rp.i;
  unsigned long long* __restrict__ bins = rp.bins;
  const int own = i < G ? labels[i] : -1;
  const bool member = own >= 0;
  rp.zero_bins(K);
  if (member) {
    const float* __restrict__ row = dist + (size_t)i * (size_t)G;
#pragma unroll 4
    for (int j = tid; j < G; j += NT) {
      const int l = labels[j];
      if (l >= 0 && j != i) atomicAdd(&bins[l], (unsigned long long)ag_kmed_q(row[j]));   // (a left-out column and the diagonal are not read)
    }
  }
  __syncthreads();
  double bm = __builtin_inf();
  int bc = 0x7fffffff;
  if (member) {
    for (int c = tid; c < K; c += NT) {             // (ascending c: a later equal mean does not replace an earlier one)
      const int n = size[c];
      if (c == own || n == 0) continue;
      ag_min_pair(bm, bc, (double)bins[c] / (double)n, c);
    }
  }
  rp.min_pair(bm, bc);
  if (tid != 0 || i >= G) return;
  if (!member) {                                    // left out
    a[i] = b[i] = s[i] = __builtin_nan("");
    other[i] = -1;
    T[i] = 0;
    return;
  }
  const int n_own = size[own];
  const bool none = bc == 0x7fffffff;
  const double ma = n_own > 1 ? (double)bins[own] / (double)(n_own - 1) : 0.0;
  const double mb = none ? 0.0 : bm;
  const double top = ma > mb ? ma : mb;
  const double si = (n_own == 1 || none || top == 0.0) ? 0.0 : (mb - ma) / top;
  a[i] = ma * (1.0 / 268435456.0);
  b[i] = none ? __builtin_nan("") : mb * (1.0 / 268435456.0);
  s[i] = si;
  other[i] = none ? -1 : bc;
  T[i] = (int64_t)__builtin_rint(si * 1099511627776.0);      // (|s| <= 1: the product is exact and the integer <= 2^40)
}

__global__ void __launch_bounds__(1024) k_sil_finish(int G, int K, const int32_t* __restrict__ labels, const int64_t* __restrict__ T,
                                                     const int32_t* __restrict__ size, double* __restrict__ cluster_mean,
                                                     double* __restrict__ mean, int32_t* __restrict__ status,
                                                     const int32_t* __restrict__ ctl) {
  if (ctl[KM_STATUS] == 2) return;                  // a bad label: k_sil_init wrote everything
  __shared__ unsigned long long s_sum[AGDIFF_PRUNE_MAX_CONFS];
  __shared__ unsigned long long s_part[16];
  __shared__ int s_cnt[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  for (int r = t; r < K; r += 1024) s_sum[r] = 0ull;
  __syncthreads();
  uint64_t total = 0;                               // (int64 sums in two's complement: the adds wrap the same way)
  int members = 0;
  for (int j = t; j < G; j += 1024) {
    const int l = labels[j];
    if (l >= 0) {
      const uint64_t v = (uint64_t)T[j];
      atomicAdd(&s_sum[l], (unsigned long long)v);
      total += v;
      ++members;
    }
  }
  ag_wave_sum(total, members);
  if (lane == 0) { s_part[wv] = total; s_cnt[wv] = members; }
  __syncthreads();
  for (int r = t; r < K; r += 1024) {
    const int n = size[r];
    cluster_mean[r] = n > 0 ? ((double)(int64_t)s_sum[r] / (double)n) * (1.0 / 1099511627776.0) : __builtin_nan("");
  }
  if (t == 0) {
    uint64_t all = 0;
    int n = 0;
    for (int w = 0; w < 16; ++w) { all += s_part[w]; n += s_cnt[w]; }
    mean[0] = n > 0 ? ((double)(int64_t)all / (double)n) * (1.0 / 1099511627776.0) : __builtin_nan("");
    status[0] = 0;
  }
}

// PAM (BUILD + SWAP) over the same float matrix (the rule: include/agdiff_hip.h, agdiff_pam_build / agdiff_pam_swap).  Again a
// sequence of launches with the kernel boundary as the only grid-wide ordering:
//   k_pam_swap_init   one workgroup: agdiff_kmedoids' seed check under the explicit anchor (ag_kmed_check_seeds)
//   k_pam_build_init  one workgroup: the anchor, the eligible count against K, tag and dn = 2^40 ("no medoid yet": with it rank 0
//                     is the same arg-max of the gain as every later rank)
//   k_pam_state       the column pass keeping the second best (ag_kmed_columns<true>): labels and near, and into `work` dn, ds
//                     and tag
//   k_pam_rows        the row pass over candidate row c: gain(c) is summed in registers and reduced by shuffles; with BINS the
//                     terms of corr(c, r) go into the bin of rank r and the pairs are (delta, rank).  One record per row:
//                     recD = delta (BUILD, without bins: -gain), recR = the rank; INT64_MAX for a row that is no candidate.
//   k_pam_choose      one workgroup over the G records (ag_pam_best: lowest recD, then lowest index, by the row pass's
//                     ag_min_pair_over): a negative delta is applied and counted, anything else ends the walk with status 0
//   k_pam_build_pick  one workgroup: the same arg-min, then medoids[p], tag and dn = min(dn, Q(row c)) along the picked row
//   k_kmed_finish     size, within, cost, n_swaps, status: as it is, from the same control words
// `work`: 8 control words (KM_DONE, KM_STATUS, KM_ITERS = the swaps made), then dn, ds, recD (64-bit each), tag, recR (32-bit
// each), one per conformer.  Every kernel of a loop reads ctl[KM_DONE] first and returns when it is set.  Sums are on integers
// (<= 2^52, differences in int64), LDS atomics are adds on integers, there are no global atomics and no workgroup waits on
// another.  Every loop is counted.
#define AG_PAM_NONE 0x7fffffffffffffffll
static_assert(AGDIFF_PAM_WORK_BYTES >= KM_CTL_WORDS * 4 + AGDIFF_PRUNE_MAX_CONFS * (3 * 8 + 2 * 4), "agdiff_pam_*: control words + dn, ds, recD, tag, recR per conformer");
static_assert(AGDIFF_PAM_MAX_SWAPS <= 4095, "agdiff_pam_swap: the launches of one call");

__global__ void __launch_bounds__(1024) k_pam_swap_init(const float* __restrict__ dist, int G, int K, const int32_t* __restrict__ init,
                                                        int anchor, int32_t* __restrict__ medoids, int32_t* __restrict__ labels,
                                                        float* __restrict__ near, int32_t* __restrict__ size, double* __restrict__ within,
                                                        double* __restrict__ cost, int32_t* __restrict__ n_swaps,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ ctl) {
  ag_kmed_check_seeds(dist, G, K, init, anchor, 1, medoids, labels, near, size, within, cost, n_swaps, status, ctl);
}

__global__ void __launch_bounds__(1024) k_pam_build_init(const float* __restrict__ dist, int G, int K, int anchor,
                                                         int32_t* __restrict__ medoids, int32_t* __restrict__ labels,
                                                         float* __restrict__ near, int32_t* __restrict__ size, double* __restrict__ within,
                                                         double* __restrict__ cost, int32_t* __restrict__ n_swaps,
                                                         int32_t* __restrict__ status, int32_t* __restrict__ ctl,
                                                         uint64_t* __restrict__ dn, int32_t* __restrict__ tag) {
  __shared__ int s_n;
  const int t = threadIdx.x;
  if (t == 0) s_n = 0;
  __syncthreads();
  const bool ok = (unsigned)anchor < (unsigned)G;   // (block-uniform)
  if (ok) {
    int n = 0;
    for (int j = t; j < G; j += 1024) {
      const bool e = j == anchor || ag_kmed_valid(dist[(size_t)anchor * (size_t)G + j]);
      tag[j] = e ? 0 : -1;
      dn[j] = 1ull << 40;
      n += e ? 1 : 0;
    }
    atomicAdd(&s_n, n);
  }
  __syncthreads();
  if (ok && s_n >= K) {
    if (t < KM_CTL_WORDS) ctl[t] = 0;
    return;
  }
  ag_kmed_fill_bad(G, K, medoids, labels, near, size, within, cost, n_swaps, status, ctl);
}

// final = 0: a state of the loop (or BUILD's one), skipped once `done` is set.  final = 1: the state after the last swap, which
// runs only after a status-1 stop (after a status-0 stop the labels already belong to the returned medoids).
__global__ void __launch_bounds__(256) k_pam_state(const float* __restrict__ dist, int G, int K, int anchor,
                                                   const int32_t* __restrict__ medoids, int32_t* __restrict__ labels,
                                                   float* __restrict__ near, const int32_t* __restrict__ ctl, uint64_t* __restrict__ dn,
                                                   uint64_t* __restrict__ ds, int32_t* __restrict__ tag, int final) {
  if (final ? ctl[KM_STATUS] != 1 : ctl[KM_DONE] != 0) return;
  ag_kmed_columns<true>(dist, G, K, anchor, medoids, labels, near, dn, ds, tag);
}

template <int ROWS, bool BINS>
__global__ void __launch_bounds__(256) k_pam_rows(const float* __restrict__ dist, int G, int K, const int32_t* __restrict__ tag,
                                                  const uint64_t* __restrict__ dn, const uint64_t* __restrict__ ds,
                                                  int64_t* __restrict__ recD, int32_t* __restrict__ recR, const int32_t* __restrict__ ctl) {
  static_assert(ROWS == 4 || (ROWS == 1 && BINS), "one row per wave, or with bins one per workgroup");
  if (ctl[KM_DONE] != 0) return;                    // (grid-uniform)
  extern __shared__ unsigned long long s_bins[];    // [ROWS][K] with BINS
  __shared__ unsigned long long s_pg[4];
  const ag_row_pass<ROWS> rp(s_bins, K);
  const int NT = rp.NT, tid = rp.tid, i = rp.i;
  unsigned long long* __restrict__ bins = rp.bins;
  const int own = i < G ? tag[i] : -1;
  const bool cand = own >= 0 && (own & 1) == 0;     // eligible and not a medoid
  if (BINS) rp.zero_bins(K);
  uint64_t gain = 0;
  if (cand) {
    const float* __restrict__ row = dist + (size_t)i * (size_t)G;
#pragma unroll 4
    for (int j = tid; j < G; j += NT) {
      const int tg = tag[j];
      if (tg < 0) continue;                         // (a left-out column takes no part)
      const uint64_t x = j == i ? 0ull : ag_kmed_q(row[j]);            // (the diagonal counts as 0)
      const uint64_t d1 = dn[j], m1 = x < d1 ? x : d1;
      gain += d1 - m1;
      if (BINS) {
        const uint64_t d2 = ds[j], term = (x < d2 ? x : d2) - m1;      // (>= 0: ds >= dn)
        if (term != 0) atomicAdd(&bins[tg >> 1], (unsigned long long)term);
      }
    }
  }
  ag_wave_sum(gain);
  int64_t bd = AG_PAM_NONE;
  int br = 0x7fffffff;
  if (BINS) {
    if (ROWS == 1 && (threadIdx.x & 63) == 0) s_pg[threadIdx.x >> 6] = gain;
    __syncthreads();
    if (ROWS == 1) gain = s_pg[0] + s_pg[1] + s_pg[2] + s_pg[3];
    if (cand)
      for (int c = tid; c < K; c += NT) ag_min_pair(bd, br, (int64_t)bins[c] - (int64_t)gain, c);
    rp.min_pair(bd, br);
  } else if (cand) {
    bd = -(int64_t)gain;                            // BUILD: the largest gain is the lowest record
    br = 0;
  }
  if (tid != 0 || i >= G) return;
  recD[i] = bd;
  recR[i] = cand ? br : 0;
}

// the arg-min of the G records by one workgroup of 1024 threads: lowest recD, then lowest index; (AG_PAM_NONE, INT_MAX) when
// no row is a candidate.  Block-uniform on return.
__device__ __forceinline__ void ag_pam_best(int G, const int64_t* __restrict__ recD, int64_t& bd, int& bj) {
  bd = AG_PAM_NONE;
  bj = 0x7fffffff;
  for (int j = threadIdx.x; j < G; j += 1024) ag_min_pair(bd, bj, recD[j], j);
  ag_min_pair_over<16>(bd, bj);
}

__global__ void __launch_bounds__(1024) k_pam_choose(int G, int max_swaps, const int64_t* __restrict__ recD,
                                                     const int32_t* __restrict__ recR, int32_t* __restrict__ medoids,
                                                     int32_t* __restrict__ ctl) {
  if (ctl[KM_DONE] != 0) return;                    // (block-uniform: ctl is written only after the barrier of ag_pam_best)
  int64_t bd;
  int bj;
  ag_pam_best(G, recD, bd, bj);
  if (threadIdx.x != 0) return;
  if (bd < 0) {                                     // the exchange lowers the cost: rank recR[bj] moves to conformer bj
    medoids[recR[bj]] = bj;
    const int n = ctl[KM_ITERS] + 1;
    ctl[KM_ITERS] = n;
    if (n >= max_swaps) ctl[KM_DONE] = 1;           // (status stays 1: whether a negative exchange is left was not looked at)
  } else {
    ctl[KM_STATUS] = 0;
    ctl[KM_DONE] = 1;
  }
}

__global__ void __launch_bounds__(1024) k_pam_build_pick(const float* __restrict__ dist, int G, int p, const int64_t* __restrict__ recD,
                                                         int32_t* __restrict__ medoids, uint64_t* __restrict__ dn,
                                                         int32_t* __restrict__ tag, const int32_t* __restrict__ ctl) {
  if (ctl[KM_DONE] != 0) return;
  int64_t bd;
  int bj;
  ag_pam_best(G, recD, bd, bj);
  if (bd == AG_PAM_NONE) return;                    // (never: K <= the eligible count; block-uniform)
  const int t = threadIdx.x;
  const float* __restrict__ row = dist + (size_t)bj * (size_t)G;
  for (int o = t; o < G; o += 1024) {
    if (tag[o] < 0) continue;
    const uint64_t x = o == bj ? 0ull : ag_kmed_q(row[o]), d = dn[o];
    dn[o] = x < d ? x : d;
    if (o == bj) tag[o] = 1;
  }
  if (t == 0) medoids[p] = bj;
}

// Agglomerative linkage over the same float matrix (the rule: include/agdiff_hip.h, agdiff_linkage).  A merge depends on the one
// before it, so the tree is a SEQUENCE OF LAUNCHES again, two per merge, the kernel boundary the only grid-wide ordering:
//   k_link_head    one workgroup: the anchor, who is eligible, M, the per-slot state, the empty-tree fill of every output
//   k_link_rows    one wave per row k (the row scaffold ag_row_pass<4>, no bins): W[k][j] = Q(dist[k][j]) for the live j > k and
//                  the row's nearest neighbour (nn_key, nn_idx): the smallest key, ties to the lowest j
//   k_link_choose  one workgroup: the arg-min of (nn_key, k) over the live rows -- lowest key, lowest a, and nn_idx[a] is the
//                  lowest b --, the merge record, the list splice, size[a], live[b], the control words a, b, the counter
//   k_link_update  one wave per slot c, writers disjoint by construction: entries with b in them are never written; wave a is
//                  the only writer of (a, c), c > a, and rescans row a from the values it just made; wave c < a is the only
//                  writer of (c, a) and rescans row c only if nn_idx[c] was a or b, otherwise it compares the new (key, a) with
//                  what it holds; wave c > a writes nothing and rescans only if nn_idx[c] was b.  No wave reads what another
//                  writes in the same launch: (b, c), (c, b) and the sizes and live flags are written by k_link_choose alone.
//   k_link_order   one workgroup: the list's ranks by pointer jumping in LDS, 12 rounds
// `work`: 16 control words, nn_key, nn_idx, size, live, next, tail per slot, then at AGDIFF_LINKAGE_WORK_FIXED_BYTES the G x G
// uint64 square, of which the pairs of eligible conformers k < j are used and all of those are written by k_link_rows.
enum { LK_COUNT = 0, LK_M = 1, LK_A = 2, LK_B = 3, LK_CTL_WORDS = 16 };   // int32 words at the head of `work`
struct ag_link_work {
  int32_t* ctl; double* nn_key; int32_t *nn_idx, *csize, *live, *next, *tail; uint64_t* W;
  explicit ag_link_work(uint64_t* work)
      : ctl((int32_t*)work), nn_key((double*)(work + LK_CTL_WORDS * 4 / 8)), nn_idx((int32_t*)(nn_key + AGDIFF_PRUNE_MAX_CONFS)),
        csize(nn_idx + AGDIFF_PRUNE_MAX_CONFS), live(csize + AGDIFF_PRUNE_MAX_CONFS), next(live + AGDIFF_PRUNE_MAX_CONFS),
        tail(next + AGDIFF_PRUNE_MAX_CONFS), W(work + AGDIFF_LINKAGE_WORK_FIXED_BYTES / 8) {}
};
static_assert(AGDIFF_LINKAGE_WORK_FIXED_BYTES >= LK_CTL_WORDS * 4 + AGDIFF_PRUNE_MAX_CONFS * (8 + 5 * 4) && AGDIFF_LINKAGE_WORK_FIXED_BYTES % 8 == 0,
              "agdiff_linkage: control words + nn_key, nn_idx, size, live, next, tail per slot");
static_assert(AGDIFF_PRUNE_MAX_CONFS == 1 << 12 && AGDIFF_KMEDOIDS_MAX_DIST == 4096, "agdiff_linkage: 2^22 pairs of 2^40 fit 64 bits; 12 rounds rank a list");
static_assert(AGDIFF_LINKAGE_CUT_WORK_BYTES >= KM_CTL_WORDS * 4 + AGDIFF_PRUNE_MAX_CONFS * 8, "agdiff_linkage_cut: control words + one key per conformer");
#define AG_LINK_NONE 0x7fffffff

__device__ __forceinline__ uint64_t ag_link_join(int method, uint64_t x, uint64_t y) {
  return method == AGDIFF_LINKAGE_SINGLE ? (x < y ? x : y) : (method == AGDIFF_LINKAGE_COMPLETE ? (x > y ? x : y) : x + y);
}

// the key of two clusters of sa and sc members with pair weight w, in units of 2^-28: the conversion rounds to nearest even (exact
// below 2^53), the count is exact, the division is one correctly rounded fp64 division
__device__ __forceinline__ double ag_link_key(int method, uint64_t w, int sa, int sc) {
  const double x = (double)w;
  return method == AGDIFF_LINKAGE_AVERAGE ? x / (double)((uint64_t)sa * (uint64_t)sc) : x;
}

// row k's nearest neighbour by the wave that owns it: the smallest key over the live j > k, ties to the lowest j, from
// entry(j), the pair weight of (k, j); (inf, -1) when no live j is left
template <typename F>
__device__ __forceinline__ void ag_link_scan(const ag_link_work& w, const ag_row_pass<4>& rp, int method, int G, int k, F entry) {
  const int sk = w.csize[k];
  double bk = __builtin_inf();
  int bj = AG_LINK_NONE;
  for (int j = k + 1 + rp.tid; j < G; j += 64) {
    if (!w.live[j]) continue;
    ag_min_pair(bk, bj, ag_link_key(method, entry(j), sk, w.csize[j]), j);
  }
  rp.min_pair(bk, bj);
  if (rp.tid == 0) {
    w.nn_key[k] = bk;
    w.nn_idx[k] = bj == AG_LINK_NONE ? -1 : bj;
  }
}

__global__ void __launch_bounds__(1024) k_link_head(const float* __restrict__ dist, int G, int anchor, ag_link_work w,
                                                    int32_t* __restrict__ left, int32_t* __restrict__ right, double* __restrict__ height,
                                                    int32_t* __restrict__ size, int32_t* __restrict__ order, int32_t* __restrict__ status) {
  const int t = threadIdx.x;
  const bool ok = (unsigned)anchor < (unsigned)G;   // (block-uniform)
  int M = 0;
  for (int base = 0; base < G; base += 1024) {      // (every thread reaches every barrier)
    const int j = base + t;
    const bool e = ok && j < G && (j == anchor || ag_kmed_valid(dist[(size_t)anchor * (size_t)G + j]));
    if (j < G) {
      w.csize[j] = e ? 1 : 0;                       // (0 for good: who is eligible, after the live flags have gone)
      w.live[j] = e ? 1 : 0;
      w.next[j] = -1;
      w.tail[j] = j;
      w.nn_key[j] = __builtin_inf();
      w.nn_idx[j] = -1;
      left[j] = -1;
      right[j] = -1;
      height[j] = __builtin_nan("");
      size[j] = 0;
      order[j] = -1;
    }
    M += __syncthreads_count(e);
  }
  if (t < LK_CTL_WORDS) w.ctl[t] = t == LK_M ? M : 0;
  if (t == 0) status[0] = ok ? 0 : 2;
}

__global__ void __launch_bounds__(256) k_link_rows(const float* __restrict__ dist, int G, int method, ag_link_work w) {
  if (w.ctl[LK_M] < 2) return;                      // (nothing to merge)
  const ag_row_pass<4> rp(nullptr, 0);
  const int k = rp.i;                               // (wave-uniform)
  if (k >= G || !w.live[k]) return;
  const float* __restrict__ row = dist + (size_t)k * (size_t)G;
  uint64_t* wrow = w.W + (size_t)k * (size_t)G;
  ag_link_scan(w, rp, method, G, k, [&](int j) {
    const uint64_t q = ag_kmed_q(row[j]);
    wrow[j] = q;
    return q;
  });
}

__global__ void __launch_bounds__(1024) k_link_choose(ag_link_work w, int G, int32_t* __restrict__ left, int32_t* __restrict__ right,
                                                      double* __restrict__ height, int32_t* __restrict__ size) {
  const int t = w.ctl[LK_COUNT];
  if (t >= w.ctl[LK_M] - 1) return;                 // (block-uniform: ctl is written only after the barrier of ag_min_pair_over)
  double bk = __builtin_inf();
  int a = AG_LINK_NONE;
  for (int k = threadIdx.x; k < G; k += 1024)
    if (w.live[k] && w.nn_idx[k] >= 0) ag_min_pair(bk, a, w.nn_key[k], k);
  ag_min_pair_over<16>(bk, a);
  if (threadIdx.x != 0 || a == AG_LINK_NONE) return;     // (never none: two live clusters are a pair)
  const int b = w.nn_idx[a];
  if (b <= a || b >= G) return;                     // (never)
  const int sa = w.csize[a], sb = w.csize[b];
  left[t] = a;
  right[t] = b;
  height[t] = bk * (1.0 / 268435456.0);
  size[t] = sa + sb;
  w.next[w.tail[a]] = b;                            // b's leaves after a's
  w.tail[a] = w.tail[b];
  w.csize[a] = sa + sb;
  w.live[b] = 0;
  w.ctl[LK_A] = a;
  w.ctl[LK_B] = b;
  w.ctl[LK_COUNT] = t + 1;
}

// `it`: the number of this launch among the G - 1; merge `it` was made iff the counter has passed it
__global__ void __launch_bounds__(256) k_link_update(ag_link_work w, int G, int method, int it) {
  if (it >= w.ctl[LK_COUNT]) return;
  const ag_row_pass<4> rp(nullptr, 0);
  const int c = rp.i;                               // (wave-uniform)
  if (c >= G || !w.live[c]) return;                 // (b is dead already)
  const int a = w.ctl[LK_A], b = w.ctl[LK_B];
  uint64_t* W = w.W;
  uint64_t* wrow = W + (size_t)c * (size_t)G;
  if (c == a) {
    ag_link_scan(w, rp, method, G, a, [&](int j) {
      const uint64_t x = ag_link_join(method, wrow[j], j > b ? W[(size_t)b * (size_t)G + j] : W[(size_t)j * (size_t)G + b]);
      wrow[j] = x;
      return x;
    });
  } else if (c < a) {
    const uint64_t x = ag_link_join(method, wrow[a], wrow[b]);
    const int nn = w.nn_idx[c];
    if (rp.tid == 0) wrow[a] = x;
    if (nn == a || nn == b) {
      ag_link_scan(w, rp, method, G, c, [&](int j) { return j == a ? x : wrow[j]; });
    } else if (rp.tid == 0) {                       // the new key may be smaller, or tie with a lower index
      double bk = w.nn_key[c];
      int bj = nn;
      ag_min_pair(bk, bj, ag_link_key(method, x, w.csize[c], w.csize[a]), a);
      w.nn_key[c] = bk;
      w.nn_idx[c] = bj;
    }
  } else if (w.nn_idx[c] == b) {
    ag_link_scan(w, rp, method, G, c, [&](int j) { return wrow[j]; });
  }
}

__global__ void __launch_bounds__(1024) k_link_order(ag_link_work w, int G, int32_t* __restrict__ order) {
  __shared__ int32_t s_next[AGDIFF_PRUNE_MAX_CONFS], s_after[AGDIFF_PRUNE_MAX_CONFS];
  const int t = threadIdx.x;
  for (int j = t; j < G; j += 1024) {
    const int n = w.csize[j] > 0 ? w.next[j] : -1;
    s_next[j] = (unsigned)n < (unsigned)G ? n : -1;
    s_after[j] = s_next[j] >= 0 ? 1 : 0;            // the leaves after j in its list, so far
  }
  __syncthreads();
  for (int round = 0; round < 12; ++round) {        // pointer jumping: 2^12 >= the longest list
    int nx[4], af[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = t + e * 1024;
      nx[e] = -1;
      af[e] = 0;
      if (j < G) {
        const int n = s_next[j];
        af[e] = s_after[j] + (n >= 0 ? s_after[n] : 0);
        nx[e] = n >= 0 ? s_next[n] : -1;
      }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = t + e * 1024;
      if (j < G) { s_next[j] = nx[e]; s_after[j] = af[e]; }
    }
    __syncthreads();
  }
  const int M = w.ctl[LK_M];
  for (int j = t; j < G; j += 1024) order[j] = w.csize[j] > 0 ? M - 1 - s_after[j] : -1;
}

// The cut of a tree (agdiff_linkage_cut), one workgroup.  The number of merges to apply is the first t that fails a test, a
// block min; parent[b] = a of the applied ones sits in LDS; thread t takes the conformers 4 t .. 4 t + 3, chases each to its
// root (a parent has a lower index: at most G steps) and the root flags' prefix sum gives the ranks.  Then the control words of
// the k-medoids launches that follow: not done, status 0, n_clusters in the updates' place.
__global__ void __launch_bounds__(1024) k_link_cut(int G, const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                   const double* __restrict__ height, const int32_t* __restrict__ order, int count,
                                                   double bound, int32_t* __restrict__ medoids, int32_t* __restrict__ labels,
                                                   float* __restrict__ near, int32_t* __restrict__ size, double* __restrict__ within,
                                                   double* __restrict__ cost, int32_t* __restrict__ n_clusters,
                                                   int32_t* __restrict__ status, int32_t* __restrict__ ctl) {
  __shared__ int32_t s_parent[AGDIFF_PRUNE_MAX_CONFS], s_rank[AGDIFF_PRUNE_MAX_CONFS];
  __shared__ int32_t s_wave[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int M = 0;
  for (int base = 0; base < G; base += 1024) {      // (every thread reaches every barrier)
    const int j = base + t;
    if (j < G) s_parent[j] = -1;
    M += __syncthreads_count(j < G && order[j] >= 0);
  }
  int n_apply = G - 1, dummy = 0;
  for (int m = t; m < G - 1; m += 1024)
    if (left[m] < 0 || M - m <= count || !(height[m] <= bound)) { n_apply = m; break; }     // (M - m clusters are left before merge m)
  ag_min_pair_over<16>(n_apply, dummy);
  int bad = 0;
  for (int m = t; m < n_apply; m += 1024) {
    const int a = left[m], b = right[m];
    if (a < 0 || a >= b || b >= G || order[a] < 0 || order[b] < 0) bad = 1;
    else s_parent[b] = a;
  }
  if (__syncthreads_or(bad)) {                      // not a tree: agdiff_kmedoids' status-2 fill, and nothing after this runs
    ag_kmed_fill_bad(G, G, medoids, labels, near, size, within, cost, n_clusters, status, ctl);
    return;
  }
  int root[4], flag[4], mine = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 4 * t + e;
    root[e] = -1;
    flag[e] = 0;
    if (j < G && order[j] >= 0) {
      int r = j;
      for (int s = 0; s < G; ++s) {
        const int p = s_parent[r];
        if (p < 0) break;
        r = p;
      }
      root[e] = r;
      flag[e] = r == j ? 1 : 0;
    }
    mine += flag[e];
  }
  int incl = mine;                                  // the inclusive prefix sum of the threads' counts: the wave, then the waves
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  int before = incl - mine, total = 0;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    before += v < wv ? s_wave[v] : 0;
    total += s_wave[v];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 4 * t + e;
    if (j < G) s_rank[j] = before;
    before += flag[e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 4 * t + e;
    if (j < G) labels[j] = root[e] >= 0 ? s_rank[root[e]] : -1;
  }
  if (t < KM_CTL_WORDS) ctl[t] = t == KM_ITERS ? total : 0;
}

// the medoid of every cluster of a cut -- k-medoids' update without an incumbent, from k_kmed_costs' keys through its arg-min --
// and near relative to it, as ag_kmed_columns writes it; the ranks past the last cluster get -1
__global__ void __launch_bounds__(1024) k_link_medoids(const float* __restrict__ dist, int G, const int32_t* __restrict__ labels,
                                                       const uint64_t* __restrict__ keys, int32_t* __restrict__ medoids,
                                                       float* __restrict__ near, const int32_t* __restrict__ ctl) {
  if (ctl[KM_DONE] != 0) return;                    // (not a tree: k_link_cut wrote everything)
  __shared__ unsigned long long s_best[AGDIFF_PRUNE_MAX_CONFS];
  const int t = threadIdx.x;
  ag_kmed_best(G, G, labels, keys, s_best);
  for (int r = t; r < G; r += 1024) medoids[r] = s_best[r] == ~0ull ? -1 : (int)(s_best[r] & 4095);
  for (int j = t; j < G; j += 1024) {
    const int l = labels[j];
    float x = __builtin_nanf("");
    if (l >= 0) {
      const int m = (int)(s_best[l] & 4095);
      x = dist[(size_t)m * (size_t)G + j];
      x = (m == j || x == 0.0f) ? 0.0f : x;         // (-0 is written as +0)
    }
    near[j] = x;
  }
}

// eigen-decomposition of the symmetric 4x4 matrix k (upper triangle as in ag_horn_key) by ag_jacobi4 with the rotations
// accumulated: returns the largest eigenvalue and its unit eigenvector q
__device__ double ag_eigvec_max4(const double (&k)[10], double (&q)[4]) {
  double d[4], V[4][4];
  ag_jacobi4<true>(k, d, V);
  double lam = d[0];
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] = V[r][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    const bool up = d[j] > lam;
    lam = up ? d[j] : lam;
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = up ? V[r][j] : q[r];
  }
  const double nrm = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int r = 0; r < 4; ++r) q[r] *= nrm;
  return lam;
}

// one wave per conformer, shaped like k_center_selected: centroids and the cross-covariance over the selected atoms in fp64
// (reduced across lanes, so every lane solves the same 4x4 problem), Horn's quaternion of lambda_max -> a proper rotation R,
// out = R (x - c_x) + c_target for ALL n atoms; rmsd = the identity-mapping RMSD of the stored coordinates over the selection
__global__ void __launch_bounds__(64) k_align_conformers(const float* __restrict__ pos, const int32_t* __restrict__ idx,
                                                         const float* __restrict__ target, int n, int m, float* __restrict__ out,
                                                         float* __restrict__ rmsd) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const float* p = pos + (size_t)g * n * 3;
  double c[6] = {0, 0, 0, 0, 0, 0};
  for (int k = lane; k < m; k += 64) {
    const int a = idx[k];
    c[0] += p[3 * a]; c[1] += p[3 * a + 1]; c[2] += p[3 * a + 2];
    c[3] += target[3 * a]; c[4] += target[3 * a + 1]; c[5] += target[3 * a + 2];
  }
  ag_wave_sum(c);
#pragma unroll
  for (int e = 0; e < 6; ++e) c[e] /= m;
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = lane; k < m; k += 64) {
    const int a = idx[k];
    const double x0 = p[3 * a] - c[0], x1 = p[3 * a + 1] - c[1], x2 = p[3 * a + 2] - c[2];
    const double y0 = target[3 * a] - c[3], y1 = target[3 * a + 1] - c[4], y2 = target[3 * a + 2] - c[5];
    ag_cov_add(S, x0, x1, x2, y0, y1, y2);
  }
  ag_wave_sum(S);
  double K[10], q[4];
  ag_horn_key(S, K);
  ag_eigvec_max4(K, q);
  const double q0 = q[0], qx = q[1], qy = q[2], qz = q[3];
  const double R[9] = {q0 * q0 + qx * qx - qy * qy - qz * qz, 2.0 * (qx * qy - q0 * qz), 2.0 * (qx * qz + q0 * qy),
                       2.0 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2.0 * (qy * qz - q0 * qx),
                       2.0 * (qz * qx - q0 * qy), 2.0 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz};
  float* o = out + (size_t)g * n * 3;
  for (int a = lane; a < n; a += 64) {
    const double x0 = p[3 * a] - c[0], x1 = p[3 * a + 1] - c[1], x2 = p[3 * a + 2] - c[2];
    o[3 * a] = (float)(R[0] * x0 + R[1] * x1 + R[2] * x2 + c[3]);
    o[3 * a + 1] = (float)(R[3] * x0 + R[4] * x1 + R[5] * x2 + c[4]);
    o[3 * a + 2] = (float)(R[6] * x0 + R[7] * x1 + R[8] * x2 + c[5]);
  }
  if (!rmsd) return;
  double d2 = 0.0;
  for (int k = lane; k < m; k += 64) {            // (another lane stored atom idx[k]: recomputed here, rounded as it was stored)
    const int a = idx[k];
    const double x0 = p[3 * a] - c[0], x1 = p[3 * a + 1] - c[1], x2 = p[3 * a + 2] - c[2];
    const double e0 = (double)(float)(R[0] * x0 + R[1] * x1 + R[2] * x2 + c[3]) - target[3 * a];
    const double e1 = (double)(float)(R[3] * x0 + R[4] * x1 + R[5] * x2 + c[4]) - target[3 * a + 1];
    const double e2 = (double)(float)(R[6] * x0 + R[7] * x1 + R[8] * x2 + c[5]) - target[3 * a + 2];
    d2 += e0 * e0 + e1 * e1 + e2 * e2;
  }
  ag_wave_sum(d2);
  if (lane == 0) rmsd[g] = (float)sqrt(d2 / m);
}

// Rigid core hold of the sampler: the selected atoms of graph g are replaced by the template's selected atoms,
// superposed on where they are now -- k_traj_rmsd's walk over a packed batch (one wave per graph, lanes striding over the graph's
// atoms whatever their number) with k_align_conformers' rotation and write-back.  Centroids, cross-covariance and norms in fp64
// from the stored fp32 coordinates; S = sum t x^T, so that Horn's quaternion of lambda_max is the proper rotation R that takes the
// centred template onto the centred core: fit = R (t - c_t) + c_x, and pos <- pos + weight (fit - pos) for the selected atoms
// only, rounded to fp32 once (weight == 1: fit itself).  pos is read AND written, through one pointer: every load that feeds the
// sums is consumed by ag_wave_sum before R exists, and the stores need R; the blend reads an atom in the lane that writes it.
// A graph with skip[g] != 0, without a selected atom or with a selected coordinate of either side that is not finite is not
// written at all and gets dev = NaN.
__global__ void __launch_bounds__(64) k_hold_core(float* pos, const float* __restrict__ core, const uint8_t* __restrict__ select,
                                                  const int32_t* __restrict__ graph_ptr, const int32_t* __restrict__ skip, int N,
                                                  float weight, float* copy_out, float* __restrict__ dev) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const float nan = __int_as_float(0x7fc00000);
  if (skip && skip[g] != 0) {                     // (wave-uniform)
    if (dev && lane == 0) dev[g] = nan;
    return;
  }
  int a0, a1;
  ag_graph_span(graph_ptr, g, N, a0, a1);
  double c[7] = {0, 0, 0, 0, 0, 0, 0};            // sums of the core's and the template's selected atoms, and their number
  for (int a = a0 + lane; a < a1; a += 64) {
    if (!select[a]) continue;
    const size_t o = (size_t)3 * a;
    c[0] += pos[o]; c[1] += pos[o + 1]; c[2] += pos[o + 2];
    c[3] += core[o]; c[4] += core[o + 1]; c[5] += core[o + 2];
    c[6] += 1.0;
  }
  ag_wave_sum(c);
  const double m = c[6];
  bool ok = m > 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) ok = ok && ag_finite(c[e]);
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, gsum = 0.0;
  const double cx = c[0] / m, cy = c[1] / m, cz = c[2] / m, tx = c[3] / m, ty = c[4] / m, tz = c[5] / m;
  if (ok) {                                       // (wave-uniform: every lane holds the same sums)
    for (int a = a0 + lane; a < a1; a += 64) {
      if (!select[a]) continue;
      const size_t o = (size_t)3 * a;
      const double x0 = pos[o] - cx, x1 = pos[o + 1] - cy, x2 = pos[o + 2] - cz;
      const double t0 = core[o] - tx, t1 = core[o + 1] - ty, t2 = core[o + 2] - tz;
      ag_cov_add(S, t0, t1, t2, x0, x1, x2);
      gsum += (x0 * x0 + x1 * x1 + x2 * x2) + (t0 * t0 + t1 * t1 + t2 * t2);
    }
    ag_wave_sum(S);
    ag_wave_sum(gsum);
    ok = ag_finite(gsum);
  }
  if (!ok) {
    if (dev && lane == 0) dev[g] = nan;
    return;
  }
  double K[10], q[4];
  ag_horn_key(S, K);
  const double lam = ag_eigvec_max4(K, q);
  const double q0 = q[0], qx = q[1], qy = q[2], qz = q[3];
  const double R[9] = {q0 * q0 + qx * qx - qy * qy - qz * qz, 2.0 * (qx * qy - q0 * qz), 2.0 * (qx * qz + q0 * qy),
                       2.0 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2.0 * (qy * qz - q0 * qx),
                       2.0 * (qz * qx - q0 * qy), 2.0 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz};
  const bool hard = weight == 1.0f;
  const double w = weight;
  for (int a = a0 + lane; a < a1; a += 64) {
    if (!select[a]) continue;
    const size_t o = (size_t)3 * a;
    const double t0 = core[o] - tx, t1 = core[o + 1] - ty, t2 = core[o + 2] - tz;
    double f0 = R[0] * t0 + R[1] * t1 + R[2] * t2 + cx;
    double f1 = R[3] * t0 + R[4] * t1 + R[5] * t2 + cy;
    double f2 = R[6] * t0 + R[7] * t1 + R[8] * t2 + cz;
    if (!hard) {
      const double p0 = pos[o], p1 = pos[o + 1], p2 = pos[o + 2];
      f0 = p0 + w * (f0 - p0); f1 = p1 + w * (f1 - p1); f2 = p2 + w * (f2 - p2);
    }
    const float v0 = (float)f0, v1 = (float)f1, v2 = (float)f2;
    pos[o] = v0; pos[o + 1] = v1; pos[o + 2] = v2;
    if (copy_out) { copy_out[o] = v0; copy_out[o + 1] = v1; copy_out[o + 2] = v2; }
  }
  if (dev && lane == 0) dev[g] = (float)sqrt(fmax((gsum - 2.0 * lam) / m, 0.0));
}

// Distance restraints of the sampler: flat-bottomed windows [lo, hi] on interatomic distances, k_hold_core's walk
// over a packed batch with a gather over the by-atom table of validity.bounds_csr.  One row of that table, for atom a at x (fp64
// from the stored fp32): worst = the largest |e| of the row, sum = sum s (-e) (x_a - x_b) / d over its entries, moved = some entry
// contributed, bad = a coordinate or a distance that is not finite.  A partner outside the graph's atoms [a0, a1) is not read.
__device__ __forceinline__ void ag_restrain_row(const float* pos, const double (&x)[3], bool a_fixed, int a0, int a1, int r0, int r1,
                                                const int32_t* __restrict__ rs_idx, const float* __restrict__ rs_lo,
                                                const float* __restrict__ rs_hi, const uint8_t* __restrict__ fixed, double (&sum)[3],
                                                double& worst, bool& moved, bool& bad) {
  bad = bad || !(ag_finite(x[0]) && ag_finite(x[1]) && ag_finite(x[2]));
  for (int r = r0; r < r1; ++r) {
    const int b = rs_idx[r];
    if ((unsigned)(b - a0) >= (unsigned)(a1 - a0)) continue;
    const size_t p = (size_t)3 * b;
    const double dx = x[0] - pos[p], dy = x[1] - pos[p + 1], dz = x[2] - pos[p + 2];
    const double d = sqrt(dx * dx + dy * dy + dz * dz);
    if (!ag_finite(d)) { bad = true; continue; }
    const double lo = rs_lo[r], hi = rs_hi[r];
    const double e = d > hi ? d - hi : (d < lo ? d - lo : 0.0);
    worst = fmax(worst, fabs(e));
    if (e == 0.0 || d < 1e-12 || a_fixed) continue;
    const double f = -((fixed && fixed[b]) ? 1.0 : 0.5) * e / d;
    sum[0] += f * dx; sum[1] += f * dy; sum[2] += f * dz;
    moved = true;
  }
}

// One wave per graph, lanes striding over the graph's atoms in rounds of 64 (every lane makes every round: the ballots below are
// wave-wide), each lane gathering the row of its own atom.  pos is read AND written in place, and a lane that strides to a later
// atom must still read pre-sweep values (Jacobi): a sweep's new values wait in LDS, at the atom's ordinal among the graph's
// restrained atoms, until every read of the sweep is done, and go out after the barrier.  A graph with skip[g] != 0, with a
// restrained coordinate that is not finite or with more than AGDIFF_RESTRAIN_MAX_ATOMS restrained atoms is not written at all and
// gets viol = NaN.  An atom whose row moved nothing keeps its bits.
__global__ void __launch_bounds__(64) k_restrain_pairs(float* pos, const int32_t* __restrict__ graph_ptr, const int32_t* __restrict__ rs_ptr,
                                                       const int32_t* __restrict__ rs_idx, const float* __restrict__ rs_lo,
                                                       const float* __restrict__ rs_hi, const uint8_t* __restrict__ fixed,
                                                       const int32_t* __restrict__ skip, int N, int R2, float weight, int sweeps,
                                                       float* copy_out, float* __restrict__ viol) {
  __shared__ float stage[3 * AGDIFF_RESTRAIN_MAX_ATOMS];
  const int g = blockIdx.x, lane = threadIdx.x;
  const float nan = __int_as_float(0x7fc00000);
  if (skip && skip[g] != 0) {                     // (wave-uniform)
    if (viol && lane == 0) viol[g] = nan;
    return;
  }
  int a0, a1;
  ag_graph_span(graph_ptr, g, N, a0, a1);
  const uint64_t below = (1ull << lane) - 1ull;
  double worst = 0.0;
  bool bad = false;
  int count = 0;
  for (int base = a0; base < a1; base += 64) {    // the measure: nothing is written before it is complete
    const int a = base + lane;
    int r0 = 0, r1 = 0;
    if (a < a1) { r0 = max(rs_ptr[a], 0); r1 = min(rs_ptr[a + 1], R2); }
    const bool has = r1 > r0;
    if (has) {
      const size_t o = (size_t)3 * a;
      const double x[3] = {pos[o], pos[o + 1], pos[o + 2]};
      double sum[3] = {0, 0, 0};
      bool moved = false;
      ag_restrain_row(pos, x, true, a0, a1, r0, r1, rs_idx, rs_lo, rs_hi, fixed, sum, worst, moved, bad);
    }
    count += __popcll(__ballot(has));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o));
  if (__ballot(bad) != 0 || count > AGDIFF_RESTRAIN_MAX_ATOMS) {            // (wave-uniform)
    if (viol && lane == 0) viol[g] = nan;
    return;
  }
  if (viol && lane == 0) viol[g] = (float)worst;
  const double w = weight;
  for (int s = 0; s < sweeps; ++s) {
    int first = 0;                                // ordinal of the round's first restrained atom
    for (int base = a0; base < a1; base += 64) {
      const int a = base + lane;
      int r0 = 0, r1 = 0;
      if (a < a1) { r0 = max(rs_ptr[a], 0); r1 = min(rs_ptr[a + 1], R2); }
      const bool has = r1 > r0;
      const uint64_t m = __ballot(has);
      if (has) {
        const size_t o = (size_t)3 * a;
        const float p0 = pos[o], p1 = pos[o + 1], p2 = pos[o + 2];
        const double x[3] = {p0, p1, p2};
        double sum[3] = {0, 0, 0}, unused = 0.0;
        bool moved = false, ignored = false;
        ag_restrain_row(pos, x, fixed && fixed[a], a0, a1, r0, r1, rs_idx, rs_lo, rs_hi, fixed, sum, unused, moved, ignored);
        const double wc = w / (double)(r1 - r0);
        const int k = 3 * (first + __popcll(m & below));
        stage[k] = moved ? (float)(x[0] + wc * sum[0]) : p0;
        stage[k + 1] = moved ? (float)(x[1] + wc * sum[1]) : p1;
        stage[k + 2] = moved ? (float)(x[2] + wc * sum[2]) : p2;
      }
      first += __popcll(m);
    }
    __syncthreads();                              // every read of the sweep is done
    const bool last = s == sweeps - 1;
    first = 0;
    for (int base = a0; base < a1; base += 64) {
      const int a = base + lane;
      const bool has = a < a1 && min(rs_ptr[a + 1], R2) > max(rs_ptr[a], 0);
      const uint64_t m = __ballot(has);
      if (has) {
        const size_t o = (size_t)3 * a;
        const int k = 3 * (first + __popcll(m & below));
        const float v0 = stage[k], v1 = stage[k + 1], v2 = stage[k + 2];
        pos[o] = v0; pos[o + 1] = v1; pos[o + 2] = v2;
        if (last && copy_out) { copy_out[o] = v0; copy_out[o + 1] = v1; copy_out[o + 2] = v2; }
      }
      first += __popcll(m);
    }
    __syncthreads();                              // the next sweep reads what this one wrote
  }
}

// Torsion restraints of the sampler: circular windows centre +- half on dihedrals.  The dihedral of the quad
// (a, u, v, b) with k_torsion_angles' arithmetic (fp64 from the fp32 positions), for batch-level atoms of the graph [a0, a1):
// 0 = an angle, 1 = degenerate (an atom outside the graph, which reads nothing, or a zero normal), 2 = a coordinate that is not
// finite.  pu, pv: the axis ends, for the rotation.
__device__ __forceinline__ int ag_quad_angle(const float* pos, int a0, int a1, int a, int u, int v, int b, double& theta, double (&pu)[3],
                                             double (&pv)[3]) {
  theta = (double)NAN;
  const unsigned n = (unsigned)(a1 - a0);
  if ((unsigned)(a - a0) >= n || (unsigned)(u - a0) >= n || (unsigned)(v - a0) >= n || (unsigned)(b - a0) >= n) return 1;
  const size_t oa = (size_t)3 * a, ou = (size_t)3 * u, ov = (size_t)3 * v, ob = (size_t)3 * b;
  const double ax = pos[oa], ay = pos[oa + 1], az = pos[oa + 2];
  pu[0] = pos[ou]; pu[1] = pos[ou + 1]; pu[2] = pos[ou + 2];
  pv[0] = pos[ov]; pv[1] = pos[ov + 1]; pv[2] = pos[ov + 2];
  const double bx = pos[ob], by = pos[ob + 1], bz = pos[ob + 2];
  if (!(ag_finite(ax) && ag_finite(ay) && ag_finite(az) && ag_finite(pu[0]) && ag_finite(pu[1]) && ag_finite(pu[2]) &&
        ag_finite(pv[0]) && ag_finite(pv[1]) && ag_finite(pv[2]) && ag_finite(bx) && ag_finite(by) && ag_finite(bz)))
    return 2;
  const double b1x = pu[0] - ax, b1y = pu[1] - ay, b1z = pu[2] - az;
  const double b2x = pv[0] - pu[0], b2y = pv[1] - pu[1], b2z = pv[2] - pu[2];
  const double b3x = bx - pv[0], b3y = by - pv[1], b3z = bz - pv[2];
  const double n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
  const double n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
  const double n1sq = n1x * n1x + n1y * n1y + n1z * n1z, n2sq = n2x * n2x + n2y * n2y + n2z * n2z;
  if (!(n1sq > 0.0 && n2sq > 0.0)) return 1;
  const double y = sqrt(b2x * b2x + b2y * b2y + b2z * b2z) * (b1x * n2x + b1y * n2y + b1z * n2z);
  const double x = n1x * n2x + n1y * n2y + n1z * n2z;
  theta = atan2(y, x);
  return 0;
}

// the excess of theta over the circular window centre +- half: 0 inside, else Delta - sign(Delta) half with Delta = theta - centre
// wrapped into [-pi, pi] (|centre| <= pi on the host, so one turn either way is enough)
__device__ __forceinline__ double ag_window_excess(double theta, double centre, double half) {
  const double pi = 3.141592653589793238462;
  double d = theta - centre;
  if (d > pi) d -= 2.0 * pi;
  else if (d < -pi) d += 2.0 * pi;
  if (fabs(d) <= half) return 0.0;
  return d > 0.0 ? d - half : d + half;
}

// One wave per graph of a packed batch.  The measure: lanes stride over the graph's restraints, nothing is written to pos before
// it is complete; a graph with skip[g] != 0 or with a quad coordinate that is not finite is not written at all, viol = NaN (and
// its angles NaN).  Then, with turn != 0, the wave walks the restraints in row order as k_flip_double_bonds walks its bonds: every
// lane computes the quad (the same loads in every lane, so the decision is wave-uniform), lane 0 stores the angle as it is when
// the restraint's turn comes, and a violated restraint with a side row has that row's atoms -- offsets from the graph's first
// atom, so every conformer of a molecule shares the row -- turned by phi = -weight e about the axis through p_v along
// k = (p_v - p_u) / |p_v - p_u|: r' = r cos phi + (k x r) sin phi + k (k . r) (1 - cos phi), r = p - p_v, in fp64, rounded to
// fp32 once.  u and v lie on the axis and are skipped; so are an offset outside the graph and an atom with a coordinate that is
// not finite.  pos is read AND written through one pointer (neither const nor __restrict__): within one restraint every
// coordinate is read and written by the same lane, the quad's loads come before the stores in the wave's program order, and a
// workgroup barrier after a rotation (wave-uniform) makes it visible to the next restraint's loads.  The workgroup is ONE wave.
__global__ void __launch_bounds__(64) k_restrain_torsions(float* pos, const int32_t* __restrict__ graph_ptr, const int32_t* __restrict__ tr_ptr,
                                                          const int32_t* __restrict__ quads, const float* __restrict__ centre,
                                                          const float* __restrict__ half, const int32_t* __restrict__ side_row,
                                                          const int32_t* __restrict__ side_ptr, const int32_t* __restrict__ side_idx,
                                                          const int32_t* __restrict__ skip, int N, int T, int S, float weight, int turn,
                                                          float* copy_out, float* __restrict__ angle, float* __restrict__ viol) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const float nan = __int_as_float(0x7fc00000);
  int a0, a1;
  ag_graph_span(graph_ptr, g, N, a0, a1);
  const int t0 = max(tr_ptr[g], 0), t1 = min(tr_ptr[g + 1], T);
  const bool skipped = skip && skip[g] != 0;      // (wave-uniform)
  double worst = 0.0, pu[3], pv[3];
  bool bad = false;
  if (!skipped) {
    for (int t = t0 + lane; t < t1; t += 64) {    // the measure
      double theta;
      const int st = ag_quad_angle(pos, a0, a1, quads[4 * t], quads[4 * t + 1], quads[4 * t + 2], quads[4 * t + 3], theta, pu, pv);
      bad = bad || st == 2;
      if (st == 0) worst = fmax(worst, fabs(ag_window_excess(theta, centre[t], half[t])));
      if (angle && !turn) angle[t] = (float)theta;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o));
  }
  if (skipped || __ballot(bad) != 0) {            // (wave-uniform)
    if (lane == 0) viol[g] = nan;
    if (angle)
      for (int t = t0 + lane; t < t1; t += 64) angle[t] = nan;
    return;
  }
  if (lane == 0) viol[g] = (float)worst;
  if (!turn) return;
  const int send = (S > 0 && side_ptr && side_idx) ? side_ptr[S] : 0;
  const double w = weight;
  for (int t = t0; t < t1; ++t) {
    const int u = quads[4 * t + 1], v = quads[4 * t + 2];
    double theta;
    const int st = ag_quad_angle(pos, a0, a1, quads[4 * t], u, v, quads[4 * t + 3], theta, pu, pv);
    if (angle && lane == 0) angle[t] = (float)theta;
    if (st != 0) continue;
    const double e = ag_window_excess(theta, centre[t], half[t]);
    const int row = side_row[t];
    if (e == 0.0 || (unsigned)row >= (unsigned)S) continue;
    const int s0 = max(side_ptr[row], 0), s1 = min(side_ptr[row + 1], send);
    if (s1 <= s0) continue;                       // (all of these wave-uniform; the normals are not zero here, so |p_v - p_u| > 0)
    const double kx0 = pv[0] - pu[0], ky0 = pv[1] - pu[1], kz0 = pv[2] - pu[2];
    const double inv = 1.0 / sqrt(kx0 * kx0 + ky0 * ky0 + kz0 * kz0);
    const double kx = kx0 * inv, ky = ky0 * inv, kz = kz0 * inv;
    double sn, cs;
    sincos(-w * e, &sn, &cs);
    for (int k = s0 + lane; k < s1; k += 64) {
      const int off = side_idx[k];
      if ((unsigned)off >= (unsigned)(a1 - a0)) continue;
      const int m = a0 + off;
      if (m == u || m == v) continue;
      const size_t o = (size_t)3 * m;
      const double rx = (double)pos[o] - pv[0], ry = (double)pos[o + 1] - pv[1], rz = (double)pos[o + 2] - pv[2];
      if (!(ag_finite(rx) && ag_finite(ry) && ag_finite(rz))) continue;
      const double kr = (kx * rx + ky * ry + kz * rz) * (1.0 - cs);
      const float v0 = (float)(pv[0] + rx * cs + (ky * rz - kz * ry) * sn + kx * kr);
      const float v1 = (float)(pv[1] + ry * cs + (kz * rx - kx * rz) * sn + ky * kr);
      const float v2 = (float)(pv[2] + rz * cs + (kx * ry - ky * rx) * sn + kz * kr);
      pos[o] = v0; pos[o + 1] = v1; pos[o + 2] = v2;
      if (copy_out) { copy_out[o] = v0; copy_out[o + 1] = v1; copy_out[o + 2] = v2; }
    }
    __syncthreads();
  }
}

// ---- handedness: the sampler cannot tell a molecule from its mirror image (the score network sees distances only), so the RMSD
// to the mirror image, the parity of the stereocentres and the inversion of a wrong-handed conformer live here ----------------

// one wave per conformer, lanes over the stereocentres (strided past 64): the signed volume of each centre's four neighbours in
// fp64, its sign against the target, and the three "some checked centre ..." facts combined across the wave by ballot.
// A quad that names an atom outside [0, n) counts as a flat centre (volume 0) and reads nothing.
__global__ void __launch_bounds__(64) k_chiral_verdict(const float* __restrict__ pos, const int32_t* __restrict__ quads,
                                                       const int8_t* __restrict__ target, int n, int C, float* __restrict__ vol,
                                                       int32_t* __restrict__ verdict) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const float* p = pos + (size_t)g * n * 3;
  bool match = false, inverted = false, flat = false;
  for (int c = lane; c < C; c += 64) {
    const int a = quads[4 * c], b = quads[4 * c + 1], d = quads[4 * c + 2], e = quads[4 * c + 3];
    double v = 0.0;
    if (ag_atoms_in_range(n, a, b, d, e)) {
      const double ax = p[3 * a], ay = p[3 * a + 1], az = p[3 * a + 2];
      const double ux = p[3 * b] - ax, uy = p[3 * b + 1] - ay, uz = p[3 * b + 2] - az;
      const double vx = p[3 * d] - ax, vy = p[3 * d + 1] - ay, vz = p[3 * d + 2] - az;
      const double wx = p[3 * e] - ax, wy = p[3 * e + 1] - ay, wz = p[3 * e + 2] - az;
      v = ux * (vy * wz - vz * wy) + uy * (vz * wx - vx * wz) + uz * (vx * wy - vy * wx);
    }
    if (vol) vol[(size_t)g * C + c] = (float)v;
    const int parity = (v > 0.0 && v <= 1.79769313486231570e308) ? 1 : ((v < 0.0 && v >= -1.79769313486231570e308) ? -1 : 0);
    const int want = target[c];
    if (want != 0) {
      flat |= parity == 0;
      match |= parity != 0 && parity == (want > 0 ? 1 : -1);
      inverted |= parity != 0 && parity != (want > 0 ? 1 : -1);
    }
  }
  const bool any_match = __ballot(match) != 0, any_inverted = __ballot(inverted) != 0, any_flat = __ballot(flat) != 0;
  if (lane == 0) verdict[g] = (any_flat || (any_match && any_inverted)) ? 0 : (any_inverted ? -1 : 1);
}

// one wave per flagged conformer, reduced as in k_center_selected: the centroid of ALL n atoms in fp64, then every coordinate
// inverted through it in place (each coordinate is read and written by the same lane); unflagged conformers are not touched
__global__ void __launch_bounds__(64) k_mirror_conformers(float* __restrict__ pos, const int32_t* __restrict__ flags, int n) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (flags[g] == 0) return;                  // (wave-uniform)
  float* p = pos + (size_t)g * n * 3;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int a = lane; a < n; a += 64) { sx += p[3 * a]; sy += p[3 * a + 1]; sz += p[3 * a + 2]; }
  ag_wave_sum(sx, sy, sz);
  const double cx2 = 2.0 * (sx / n), cy2 = 2.0 * (sy / n), cz2 = 2.0 * (sz / n);
  for (int a = lane; a < n; a += 64) {
    p[3 * a] = (float)(cx2 - (double)p[3 * a]);
    p[3 * a + 1] = (float)(cy2 - (double)p[3 * a + 1]);
    p[3 * a + 2] = (float)(cz2 - (double)p[3 * a + 2]);
  }
}

// E/Z of double bonds: one wave per conformer, which walks the D tagged bonds in row order.  Every lane computes
// n1 . n2 of the quad (a, i, j, e) with k_torsion_angles' arithmetic (fp64 from the fp32 positions: the same loads in every lane, so
// the decision is wave-uniform): parity + 1 (trans) when n1 . n2 < 0, - 1 (cis) when > 0, 0 when a normal is zero or a coordinate
// is not finite; state = parity against the target's sign, 0 for target 0, written from the positions as they are when the bond's
// turn comes.  A wrong bond with a side row is flipped: the lanes stride over the row and turn each listed atom by 180 degrees
// about the axis through p_i along u = (p_j - p_i) / |p_j - p_i|, p' = 2 (p_i + u (u . (p - p_i))) - p in fp64, rounded to fp32
// once.  Atoms i and j lie on the axis and are skipped, so they stay bit for bit; so does a listed atom with a coordinate that is
// not finite or an index outside [0, n).  pos is read AND written through one pointer (neither const nor __restrict__): within
// one bond every coordinate is read and written by the same lane, the loads of the quad come before the stores in the wave's
// program order, and a workgroup barrier after a rotation (wave-uniform: state is) makes it visible to the next bond's loads.
// The workgroup is ONE wave: with more, a second barrier between a bond's quad loads and its stores would be needed.
// A conformer without a wrong bond that has a side row is not written at all.
__global__ void __launch_bounds__(64) k_flip_double_bonds(float* pos, const int32_t* __restrict__ quads, const int8_t* __restrict__ target,
                                                          const int32_t* __restrict__ side_ptr, const int32_t* __restrict__ side_idx,
                                                          int n, int D, int8_t* __restrict__ state, int32_t* __restrict__ flipped) {
  const int g = blockIdx.x, lane = threadIdx.x;
  float* p = pos + (size_t)g * n * 3;
  int count = 0;
  for (int c = 0; c < D; ++c) {
    const int a = quads[4 * c], u = quads[4 * c + 1], v = quads[4 * c + 2], b = quads[4 * c + 3];
    int parity = 0;
    double ux = 0.0, uy = 0.0, uz = 0.0, b2x = 0.0, b2y = 0.0, b2z = 0.0;
    if (ag_atoms_in_range(n, a, u, v, b)) {
      const double ax = p[3 * a], ay = p[3 * a + 1], az = p[3 * a + 2];
      ux = p[3 * u]; uy = p[3 * u + 1]; uz = p[3 * u + 2];
      const double vx = p[3 * v], vy = p[3 * v + 1], vz = p[3 * v + 2];
      const double bx = p[3 * b], by = p[3 * b + 1], bz = p[3 * b + 2];
      const double b1x = ux - ax, b1y = uy - ay, b1z = uz - az;
      b2x = vx - ux; b2y = vy - uy; b2z = vz - uz;
      const double b3x = bx - vx, b3y = by - vy, b3z = bz - vz;
      const double n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
      const double n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
      const double n1sq = n1x * n1x + n1y * n1y + n1z * n1z, n2sq = n2x * n2x + n2y * n2y + n2z * n2z;
      const double x = n1x * n2x + n1y * n2y + n1z * n2z;                    // |n1| |n2| cos(phi): phi = 0 cis, pi trans
      const bool finite = ag_finite(ax) && ag_finite(ay) && ag_finite(az) && ag_finite(ux) && ag_finite(uy) && ag_finite(uz) &&
                          ag_finite(vx) && ag_finite(vy) && ag_finite(vz) && ag_finite(bx) && ag_finite(by) && ag_finite(bz);
      if (finite && n1sq > 0.0 && n2sq > 0.0) parity = x < 0.0 ? 1 : (x > 0.0 ? -1 : 0);
    }
    const int want = target[c];
    const int st = (want == 0 || parity == 0) ? 0 : (parity == (want > 0 ? 1 : -1) ? 1 : -1);
    if (lane == 0) state[(size_t)g * D + c] = (int8_t)st;
    const int s0 = side_ptr[c], s1 = side_ptr[c + 1];
    if (st < 0 && s0 >= 0 && s1 > s0 && side_idx) {                                    // (wave-uniform; n1sq > 0 here, so |b2| > 0)
      const double inv = 1.0 / sqrt(b2x * b2x + b2y * b2y + b2z * b2z);
      const double ex = b2x * inv, ey = b2y * inv, ez = b2z * inv;
      for (int k = s0 + lane; k < s1; k += 64) {
        const int m = side_idx[k];
        if (m == u || m == v || !ag_atoms_in_range(n, m)) continue;
        const double px = p[3 * m], py = p[3 * m + 1], pz = p[3 * m + 2];
        if (!(ag_finite(px) && ag_finite(py) && ag_finite(pz))) continue;
        const double t = ex * (px - ux) + ey * (py - uy) + ez * (pz - uz);
        p[3 * m] = (float)(2.0 * (ux + ex * t) - px);
        p[3 * m + 1] = (float)(2.0 * (uy + ey * t) - py);
        p[3 * m + 2] = (float)(2.0 * (uz + ez * t) - pz);
      }
      ++count;
      __syncthreads();
    }
  }
  if (flipped && lane == 0) flipped[g] = count;
}

// ---- torsion fingerprint deviation: RMSD grows with the molecule and mixes ring breathing with rotamer changes; the dihedrals of
// the rotatable bonds are what defines a conformer, so the matrix, the threshold bits and the mirror value exist over them too ----

// The dihedral of the quad (a, u, v, b) from its twelve coordinates (fp32 values taken to fp64), theta = atan2(|b2| b1 . n2, n1 . n2):
// the ONE copy of the arithmetic, called by k_torsion_angles (coordinates from global memory) and k_ring_coords (from LDS).  NaN for
// a degenerate quad (a zero normal) or an input that is not finite.
__device__ __forceinline__ double ag_dihedral(double ax, double ay, double az, double ux, double uy, double uz, double vx, double vy,
                                              double vz, double bx, double by, double bz) {
  const double b1x = ux - ax, b1y = uy - ay, b1z = uz - az;
  const double b2x = vx - ux, b2y = vy - uy, b2z = vz - uz;
  const double b3x = bx - vx, b3y = by - vy, b3z = bz - vz;
  const double n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
  const double n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
  const double n1sq = n1x * n1x + n1y * n1y + n1z * n1z, n2sq = n2x * n2x + n2y * n2y + n2z * n2z;
  // (fp32 inputs: every difference and product above is finite in fp64 iff the twelve coordinates are; an Inf or NaN among
  // them reaches n1sq or n2sq or both of y and x below)
  const double y = sqrt(b2x * b2x + b2y * b2y + b2z * b2z) * (b1x * n2x + b1y * n2y + b1z * n2z);
  const double x = n1x * n2x + n1y * n2y + n1z * n2z;
  const bool finite = ag_finite(ax) && ag_finite(ay) && ag_finite(az) && ag_finite(ux) && ag_finite(uy) && ag_finite(uz) &&
                      ag_finite(vx) && ag_finite(vy) && ag_finite(vz) && ag_finite(bx) && ag_finite(by) && ag_finite(bz);
  return (finite && n1sq > 0.0 && n2sq > 0.0) ? atan2(y, x) : (double)NAN;
}

// one wave per conformer, lanes over the columns (strided past 64), shaped like k_chiral_verdict: the dihedral of every quad
// (a, u, v, b) in fp64 from the fp32 positions (ag_dihedral).  NaN for a degenerate quad, an input that is not finite, or a quad
// that names an atom outside [0, n), which reads nothing.
__global__ void __launch_bounds__(64) k_torsion_angles(const float* __restrict__ pos, const int32_t* __restrict__ quads, int n, int Q,
                                                       float* __restrict__ out) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const float* p = pos + (size_t)g * n * 3;
  for (int c = lane; c < Q; c += 64) {
    const int a = quads[4 * c], u = quads[4 * c + 1], v = quads[4 * c + 2], b = quads[4 * c + 3];
    double theta = (double)NAN;
    if (ag_atoms_in_range(n, a, u, v, b))
      theta = ag_dihedral(p[3 * a], p[3 * a + 1], p[3 * a + 2], p[3 * u], p[3 * u + 1], p[3 * u + 2], p[3 * v], p[3 * v + 1],
                          p[3 * v + 2], p[3 * b], p[3 * b + 1], p[3 * b + 2]);
    out[(size_t)g * Q + c] = (float)theta;
  }
}

// circular difference of two angles in radians; pi when either is NaN (a broken torsion never makes two conformers look alike)
__device__ __forceinline__ double ag_circ_diff(double d) {     // d = |alpha - beta| (or |alpha + beta| against the mirror image)
  const double r = fmin(d, 6.283185307179586476925 - d);
  return d != d ? 3.141592653589793238462 : r;
}

// 16 x 16 pairs per workgroup as in k_rmsd_matrix: thread (ty, tx) = (row conformer j0 + ty of ang_x, column conformer i0 + tx of
// ang_y).  The 16 + 16 angle rows sit in LDS at an odd pitch, so the 16 threads of a tile row, which read one column of 16
// different y rows, hit 16 different banks (the x row is a broadcast).  One thread walks the P mappings of its pair:
//   S_p(x -> y) = sum_t w_t delta(x[tmap[0][t]], y[tmap[p][t]]) / (pi sum_t w_t),  value = min_p min(S_p(x -> y), S_p(y -> x)),
// the mirror value the same with every y angle negated.  Both sums are accumulated in the same order with a delta that is
// symmetric in its arguments, so thread (x, y) and thread (y, x) of a self matrix compute each other's pair of sums bit for bit.
// bits: the layout of k_rmsd_self, R rows; the wave's ballot holds four tile rows of 16 flags, the lane with tx == 0 stores its
// row's piece, and the tiles of the last tile column zero the pad pieces of their rows.
__global__ void __launch_bounds__(256) k_tfd_matrix(const float* __restrict__ ang_x, const float* __restrict__ ang_y,
                                                    const int32_t* __restrict__ tmap, const float* __restrict__ w, int R, int G, int Q,
                                                    int T, int P, float thresh, float* __restrict__ out, float* __restrict__ out_mirror,
                                                    uint16_t* __restrict__ bits, int pitch) {
  const int lp = Q | 1;                             // LDS pitch in floats: odd
  float* sx = ag_eval_smem;
  float* sy = ag_eval_smem + 16 * lp;
  const int j0 = blockIdx.y * 16, i0 = blockIdx.x * 16;
  for (int t = threadIdx.x; t < 16 * Q; t += 256) {
    const int c = t / Q, o = t % Q;
    sx[c * lp + o] = (j0 + c < R) ? ang_x[(size_t)(j0 + c) * Q + o] : 0.0f;
    sy[c * lp + o] = (i0 + c < G) ? ang_y[(size_t)(i0 + c) * Q + o] : 0.0f;
  }
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const bool valid = j0 + ty < R && i0 + tx < G;
  float v = 0.0f, vm = 0.0f;
  if (valid && T > 0) {
    const float* x = sx + ty * lp;
    const float* y = sy + tx * lp;
    double wsum = 0.0;
    for (int t = 0; t < T; ++t) wsum += w ? (double)w[t] : 1.0;
    double best = 1e300, best_mirror = 1e300;
    for (int p = 0; p < P; ++p) {
      const int32_t* mp = tmap + (size_t)p * T;
      double sxy = 0.0, syx = 0.0, mxy = 0.0, myx = 0.0;
      for (int t = 0; t < T; ++t) {
        const int c0 = tmap[t], cp = mp[t];
        const double wt = w ? (double)w[t] : 1.0;
        const double x0 = x[c0], yp = y[cp], y0 = y[c0], xp = x[cp];
        sxy += wt * ag_circ_diff(fabs(x0 - yp));
        syx += wt * ag_circ_diff(fabs(y0 - xp));
        mxy += wt * ag_circ_diff(fabs(x0 + yp));
        myx += wt * ag_circ_diff(fabs(y0 + xp));
      }
      best = fmin(best, fmin(sxy, syx));
      best_mirror = fmin(best_mirror, fmin(mxy, myx));
    }
    const double norm = 3.141592653589793238462 * wsum;
    v = (float)(best / norm);
    vm = (float)(best_mirror / norm);
  }
  if (valid) {
    const size_t at = (size_t)(j0 + ty) * G + i0 + tx;
    if (out) out[at] = v;
    if (out_mirror) out_mirror[at] = vm;
  }
  if (bits) {                                       // (every lane of the wave arrives here)
    // the threshold is taken on the fp32 value as stored, so that bits == (out <= thresh) exactly
    const unsigned long long flags = __ballot(valid && v <= thresh);
    const int pieces = pitch >> 1, tiles_g = (G + 15) / 16;
    if (j0 + ty < R) {
      uint16_t* row = bits + (size_t)(j0 + ty) * pieces;
      if (tx == 0) row[blockIdx.x] = (uint16_t)(flags >> (16 * (ty & 3)));
      if ((int)blockIdx.x == tiles_g - 1 && tx >= 1 && tiles_g - 1 + tx < pieces) row[tiles_g - 1 + tx] = 0;
    }
  }
}

// ---- ring conformations: the rotatable bonds are bridges, so nothing above sees a ring.  The shape of every ring (the ring torsion
// value and the Cremer-Pople puckering coordinates; include/agdiff_hip.h has the definitions), and the TFD over terms that carry a
// scale and a parity of their own, so that rings stand next to bonds ----

constexpr int AG_RING_SLOTS = 512;   // (ring, position) slots of one pass of k_ring_coords: four fp64 each (16 KB of LDS) + the ring ids

// One wave per conformer, like k_torsion_angles / k_planar_groups, but a molecule has 1 .. 6 rings and one lane per ring would idle
// the wave: the lanes walk the (ring, position) slots of the table, strided past 64, in passes of whole rings of at most
// AG_RING_SLOTS slots (the launcher has checked 4 <= N <= AGDIFF_RING_MAX_ATOMS, so a ring always fits).  Per pass:
//   1  slot (r, j): the position of atom r_j as fp64 into LDS -- NaN when ANY atom of the ring is outside [0, n): the ring reads
//      nothing, and NaN positions make every number of it NaN below
//   2  slot (r, j): |theta(r_j, r_j+1, r_j+2, r_j+3)| from LDS (ag_dihedral) into LDS
//   3  one lane per ring, j ascending: tau = sum |theta_j| / N; centroid, R', R'', the normal, z_j (written over the ring's own
//      |theta_j|), Q = sqrt(sum z_j^2); z_j = NaN when |R' x R''|^2 is zero or a coordinate is not finite
//   4  slot (r, m), 2 <= m <= N / 2: the mode's sum over z_j, j ascending -> (q_m, phi_m), or the signed q_(N/2)
// Every sum is made by one lane in a fixed order from values that depend on the ring alone, so a ring's numbers do not depend on
// the launch, on which slots it occupies or on what else the table holds.  Each output has one writer.
__global__ void __launch_bounds__(64) k_ring_coords(const float* __restrict__ pos, const int32_t* __restrict__ ring_ptr,
                                                    const int32_t* __restrict__ ring_idx, int n, int Rg, float* __restrict__ tau,
                                                    float* __restrict__ amp, float* __restrict__ pucker) {
  __shared__ double sx[AG_RING_SLOTS], sy[AG_RING_SLOTS], sz[AG_RING_SLOTS], sv[AG_RING_SLOTS];
  __shared__ int16_t sring[AG_RING_SLOTS];
  const int g = blockIdx.x, lane = threadIdx.x;
  const float* p = pos + (size_t)g * n * 3;
  const size_t K = (size_t)(ring_ptr[Rg] - 3 * Rg);
  for (int r0 = 0; r0 < Rg;) {
    const int s0 = ring_ptr[r0];
    int r1 = r0 + 1;
    while (r1 < Rg && ring_ptr[r1 + 1] - s0 <= AG_RING_SLOTS) ++r1;
    const int S = ring_ptr[r1] - s0;
    if (S <= 0 || S > AG_RING_SLOTS) return;        // (a table the launcher would have refused; uniform over the wave)
    for (int r = r0 + lane; r < r1; r += 64)
      for (int s = ring_ptr[r] - s0; s < ring_ptr[r + 1] - s0; ++s) sring[s] = (int16_t)(r - r0);
    __syncthreads();
    for (int s = lane; s < S; s += 64) {            // 1
      const int r = r0 + sring[s], b = ring_ptr[r], N = ring_ptr[r + 1] - b;
      bool ok = true;
      for (int j = 0; j < N; ++j) ok = ok && ag_atoms_in_range(n, ring_idx[b + j]);
      const int a = ring_idx[s0 + s];
      sx[s] = ok ? (double)p[3 * a] : (double)NAN;
      sy[s] = ok ? (double)p[3 * a + 1] : (double)NAN;
      sz[s] = ok ? (double)p[3 * a + 2] : (double)NAN;
    }
    __syncthreads();
    for (int s = lane; s < S; s += 64) {            // 2
      const int r = r0 + sring[s], lb = ring_ptr[r] - s0, N = ring_ptr[r + 1] - s0 - lb, j = s - lb;
      const int i1 = lb + (j + 1) % N, i2 = lb + (j + 2) % N, i3 = lb + (j + 3) % N;
      sv[s] = fabs(ag_dihedral(sx[s], sy[s], sz[s], sx[i1], sy[i1], sz[i1], sx[i2], sy[i2], sz[i2], sx[i3], sy[i3], sz[i3]));
    }
    __syncthreads();
    for (int r = r0 + lane; r < r1; r += 64) {      // 3
      const int lb = ring_ptr[r] - s0, N = ring_ptr[r + 1] - s0 - lb;
      const double inv = 1.0 / N;
      double t = 0.0;
      for (int j = 0; j < N; ++j) t += sv[lb + j];
      if (tau) tau[(size_t)g * Rg + r] = (float)(t * inv);
      double cx = 0.0, cy = 0.0, cz = 0.0;
      for (int j = 0; j < N; ++j) { cx += sx[lb + j]; cy += sy[lb + j]; cz += sz[lb + j]; }
      // (fp32 values: the three sums are finite iff every coordinate of the ring is)
      const bool fin = ag_finite(cx) && ag_finite(cy) && ag_finite(cz);
      cx *= inv; cy *= inv; cz *= inv;
      double ax = 0.0, ay = 0.0, az = 0.0, bx = 0.0, by = 0.0, bz = 0.0;     // R', R''
      for (int j = 0; j < N; ++j) {
        double sn, cs;
        sincospi((double)((2 * j) % (2 * N)) * inv, &sn, &cs);
        const double dx = sx[lb + j] - cx, dy = sy[lb + j] - cy, dz = sz[lb + j] - cz;
        ax += dx * sn; ay += dy * sn; az += dz * sn;
        bx += dx * cs; by += dy * cs; bz += dz * cs;
      }
      double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
      const double nsq = nx * nx + ny * ny + nz * nz;
      const bool ok = fin && nsq > 0.0 && ag_finite(nsq);
      const double s = 1.0 / sqrt(nsq);
      nx *= s; ny *= s; nz *= s;
      double zz = 0.0;
      for (int j = 0; j < N; ++j) {
        const double z = ok ? (sx[lb + j] - cx) * nx + (sy[lb + j] - cy) * ny + (sz[lb + j] - cz) * nz : (double)NAN;
        zz += z * z;
        sv[lb + j] = z;
      }
      if (amp) amp[(size_t)g * Rg + r] = (float)sqrt(zz);
    }
    __syncthreads();
    if (pucker) {
      for (int s = lane; s < S; s += 64) {          // 4
        const int r = r0 + sring[s], lb = ring_ptr[r] - s0, N = ring_ptr[r + 1] - s0 - lb, m = s - lb;
        float* o = pucker + (size_t)g * K + (size_t)(ring_ptr[r] - 3 * r);
        if (m >= 2 && m <= (N - 1) / 2) {
          double a = 0.0, b = 0.0;
          for (int j = 0; j < N; ++j) {
            double sn, cs;
            sincospi((double)((2 * m * j) % (2 * N)) / N, &sn, &cs);
            a += sv[lb + j] * cs;
            b += sv[lb + j] * sn;
          }
          const double f = sqrt(2.0 / N);
          a *= f;
          b *= -f;
          double phi = atan2(b, a);
          if (phi < 0.0) phi += 6.283185307179586476925;
          const float ph = (float)phi;
          o[2 * (m - 2)] = (float)sqrt(a * a + b * b);
          o[2 * (m - 2) + 1] = ph >= 6.2831855f ? 0.0f : ph;       // (the fp32 nearest to 2 pi lies above it)
        } else if (!(N & 1) && m == N / 2) {
          double a = 0.0;
          for (int j = 0; j < N; ++j) a += (j & 1) ? -sv[lb + j] : sv[lb + j];
          o[N - 4] = (float)(a * sqrt(1.0 / N));
        }
      }
    }
    __syncthreads();                                // (the next pass writes the LDS this one reads)
    r0 = r1;
  }
}

// k_tfd_matrix with a scale and a parity per term (k_tfd_matrix itself is left as it is: its values are pinned bit for bit): the
// same tiles, LDS pitch, bit layout and output rules.  The T pairs (1 / s_t, the mirror's sign: +1 where a reflection leaves the
// value, -1 where it negates it) are staged in LDS as fp64 in front of the angle rows.
//   S_p(x -> y) = sum_t w_t min(1, delta(x[tmap[0][t]], y[tmap[p][t]]) (1 / s_t)) / sum_t w_t, a NaN value counting 1.
// As there, both directions accumulate in the same order with a delta that is symmetric in its arguments, so a self matrix is
// symmetric bit for bit.
__device__ __forceinline__ double ag_term_diff(double d, double rs) {     // d = |alpha - beta|, rs = 1 / s_t
  const double r = fmin(fmin(d, 6.283185307179586476925 - d) * rs, 1.0);
  return d != d ? 1.0 : r;
}

__global__ void __launch_bounds__(256) k_tfd_matrix_terms(const float* __restrict__ ang_x, const float* __restrict__ ang_y,
                                                          const int32_t* __restrict__ tmap, const float* __restrict__ w,
                                                          const float* __restrict__ scale, const int32_t* __restrict__ even, int R,
                                                          int G, int Q, int T, int P, float thresh, float* __restrict__ out,
                                                          float* __restrict__ out_mirror, uint16_t* __restrict__ bits, int pitch) {
  const int lp = Q | 1;                             // LDS pitch in floats: odd
  // [T][2] fp64 at the base of the dynamic LDS, 16 bytes a term.  ag_eval_smem is declared as float (4-byte aligned): the base is
  // 8-byte aligned because this kernel has NO static __shared__, so the dynamic segment starts at LDS offset 0.  Adding a static
  // __shared__ here would need the term pairs moved or the base rounded up.
  double* sterm = reinterpret_cast<double*>(ag_eval_smem);
  float* sx = ag_eval_smem + 4 * T;
  float* sy = sx + 16 * lp;
  const int j0 = blockIdx.y * 16, i0 = blockIdx.x * 16;
  for (int t = threadIdx.x; t < T; t += 256) {
    sterm[2 * t] = 1.0 / (double)scale[t];
    sterm[2 * t + 1] = even[t] ? 1.0 : -1.0;
  }
  for (int t = threadIdx.x; t < 16 * Q; t += 256) {
    const int c = t / Q, o = t % Q;
    sx[c * lp + o] = (j0 + c < R) ? ang_x[(size_t)(j0 + c) * Q + o] : 0.0f;
    sy[c * lp + o] = (i0 + c < G) ? ang_y[(size_t)(i0 + c) * Q + o] : 0.0f;
  }
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const bool valid = j0 + ty < R && i0 + tx < G;
  float v = 0.0f, vm = 0.0f;
  if (valid && T > 0) {
    const float* x = sx + ty * lp;
    const float* y = sy + tx * lp;
    double wsum = 0.0;
    for (int t = 0; t < T; ++t) wsum += w ? (double)w[t] : 1.0;
    double best = 1e300, best_mirror = 1e300;
    for (int p = 0; p < P; ++p) {
      const int32_t* mp = tmap + (size_t)p * T;
      double sxy = 0.0, syx = 0.0, mxy = 0.0, myx = 0.0;
      for (int t = 0; t < T; ++t) {
        const int c0 = tmap[t], cp = mp[t];
        const double wt = w ? (double)w[t] : 1.0;
        const double rs = sterm[2 * t], sg = sterm[2 * t + 1];
        const double x0 = x[c0], yp = y[cp], y0 = y[c0], xp = x[cp];
        sxy += wt * ag_term_diff(fabs(x0 - yp), rs);
        syx += wt * ag_term_diff(fabs(y0 - xp), rs);
        mxy += wt * ag_term_diff(fabs(x0 - sg * yp), rs);
        myx += wt * ag_term_diff(fabs(sg * y0 - xp), rs);
      }
      best = fmin(best, fmin(sxy, syx));
      best_mirror = fmin(best_mirror, fmin(mxy, myx));
    }
    v = (float)(best / wsum);
    vm = (float)(best_mirror / wsum);
  }
  if (valid) {
    const size_t at = (size_t)(j0 + ty) * G + i0 + tx;
    if (out) out[at] = v;
    if (out_mirror) out_mirror[at] = vm;
  }
  if (bits) {                                       // (every lane of the wave arrives here)
    // the threshold is taken on the fp32 value as stored, so that bits == (out <= thresh) exactly
    const unsigned long long flags = __ballot(valid && v <= thresh);
    const int pieces = pitch >> 1, tiles_g = (G + 15) / 16;
    if (j0 + ty < R) {
      uint16_t* row = bits + (size_t)(j0 + ty) * pieces;
      if (tx == 0) row[blockIdx.x] = (uint16_t)(flags >> (16 * (ty & 3)));
      if ((int)blockIdx.x == tiles_g - 1 && tx >= 1 && tiles_g - 1 + tx < pieces) row[tiles_g - 1 + tx] = 0;
    }
  }
}

// ---- geometry validity: a sampled conformer can be finite and still broken (a stretched bond, two rings pushed through each
// other).  Two topology-only checks: bounded pair distances, and an all-pairs clash scan that leaves out the pairs 1 .. 3 bonds apart --

// the fp64 distance of atoms a and b of one conformer from the fp32 positions
__device__ __forceinline__ double ag_pair_dist(const float* __restrict__ p, int a, int b) {
  const double dx = (double)p[3 * a] - (double)p[3 * b], dy = (double)p[3 * a + 1] - (double)p[3 * b + 1];
  const double dz = (double)p[3 * a + 2] - (double)p[3 * b + 2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// (best, best_k) of a lane = its largest value and the lowest index attaining it, best_k < 0 when it has none: afterwards every
// lane holds the wave's largest value with the lowest index attaining it, and the sum of `count` over the lanes
__device__ __forceinline__ void ag_wave_worst(float& best, int& best_k, int& count) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o);
    const int ok = __shfl_xor(best_k, o);
    count += __shfl_xor(count, o);
    if (ok >= 0 && (ov > best || (ov == best && ok < best_k))) { best = ov; best_k = ok; }
  }
}

// one wave per conformer, lanes over the pairs (strided past 64), shaped like k_torsion_angles: d as fp32, the violation
// v = max(lo - d, d - hi, 0) on that fp32 d (+inf when d is not finite), then max / lowest index / count across the lanes by
// shuffles.  A pair that names an atom outside [0, n) has d = NaN, v = +inf and reads nothing.
__global__ void __launch_bounds__(64) k_pair_bounds(const float* __restrict__ pos, const int32_t* __restrict__ pairs,
                                                    const float* __restrict__ lo, const float* __restrict__ hi, int n, int K,
                                                    float* __restrict__ dist, float* __restrict__ worst,
                                                    int32_t* __restrict__ worst_pair, int32_t* __restrict__ n_bad) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const float* p = pos + (size_t)g * n * 3;
  float best = -1.0f;                               // (below every violation: the lane's first pair is taken)
  int best_k = -1, bad = 0;
  for (int k = lane; k < K; k += 64) {
    const int a = pairs[2 * k], b = pairs[2 * k + 1];
    float d = NAN;
    if (ag_atoms_in_range(n, a, b)) d = (float)ag_pair_dist(p, a, b);
    if (dist) dist[(size_t)g * K + k] = d;
    float v = INFINITY;
    if (fabsf(d) <= 3.40282347e38f) v = (float)fmax(fmax((double)lo[k] - (double)d, (double)d - (double)hi[k]), 0.0);
    bad += v > 0.0f ? 1 : 0;
    if (v > best) { best = v; best_k = k; }         // (k ascends: the lane keeps its lowest k)
  }
  ag_wave_worst(best, best_k, bad);
  if (lane == 0) {
    worst[g] = best_k < 0 ? 0.0f : best;
    worst_pair[g] = best_k;
    n_bad[g] = bad;
  }
}

// ---- planarity: a conformer can keep every bond length and every contact legal and still fold an aromatic ring into a boat or
// twist the two ends of a double bond against each other.  The host names the groups of atoms that must lie in one plane
// (agdiff_amd/planarity.py); the check is each member's distance from the group's best plane --

// unit normal of the best plane through centred points with the covariance A = (xx xy xz yy yz zz): the eigenvector of A's smallest
// eigenvalue.  The 3x3 problem sits in the 4x4 key of ag_jacobi4 with a fourth diagonal entry no rotation touches (its row and
// column are exactly zero, ag_jacobi4 skips a zero pivot and a rotation of two other columns leaves them zero), so d[3], column 3
// and the fourth component of the other columns stay (0, e_4, 0) and are not read.
__device__ void ag_plane_normal(const double (&A)[6], double (&nrm)[3]) {
  const double k[10] = {A[0], A[1], A[2], 0.0, A[3], A[4], 0.0, A[5], 0.0, 0.0};
  double d[4], V[4][4];
  ag_jacobi4<true>(k, d, V);
  double lam = d[0];
#pragma unroll
  for (int r = 0; r < 3; ++r) nrm[r] = V[r][0];
#pragma unroll
  for (int j = 1; j < 3; ++j) {
    const bool down = d[j] < lam;
    lam = down ? d[j] : lam;
#pragma unroll
    for (int r = 0; r < 3; ++r) nrm[r] = down ? V[r][j] : nrm[r];
  }
  const double s = 1.0 / sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) nrm[r] *= s;
}

// The best plane of one group, members mem[0 .. m), coordinate c of atom a = at(a, c) as fp64: the ONE copy of the per-group
// computation, called by k_planar_groups (coordinates from global memory) and by the repair's phase A (from LDS).  The members are
// walked twice, so that no 24-double array lives in registers: once for the sums of u_k = x_k - x_0 and of u_k u_k^T (relative to
// the first member, so that the covariance A = sum u u^T / m - ubar ubar^T cancels over the group's extent and not over its
// distance from the origin), once for the projections normal . (u_k - ubar) = normal . (x_k - centroid).  org = x_0, ubar = the
// centroid relative to it, nrm = the unit normal, far = the largest |projection|.  false, and only org written, when a member
// coordinate is not finite.
template <typename F>
__device__ __forceinline__ bool ag_group_plane(F at, const int32_t* __restrict__ mem, int m, double (&org)[3], double (&ubar)[3],
                                               double (&nrm)[3], double& far) {
  const int a0 = mem[0];
  const double ox = at(a0, 0), oy = at(a0, 1), oz = at(a0, 2);
  org[0] = ox; org[1] = oy; org[2] = oz;
  double s[3] = {0, 0, 0}, S[6] = {0, 0, 0, 0, 0, 0};
  bool fin = ag_finite(ox) && ag_finite(oy) && ag_finite(oz);
  for (int j = 1; j < m; ++j) {
    const int a = mem[j];
    const double x = at(a, 0), y = at(a, 1), z = at(a, 2);
    fin = fin && ag_finite(x) && ag_finite(y) && ag_finite(z);
    const double ux = x - ox, uy = y - oy, uz = z - oz;
    s[0] += ux; s[1] += uy; s[2] += uz;
    S[0] += ux * ux; S[1] += ux * uy; S[2] += ux * uz; S[3] += uy * uy; S[4] += uy * uz; S[5] += uz * uz;
  }
  if (!fin) return false;
  const double inv = 1.0 / m, cx = s[0] * inv, cy = s[1] * inv, cz = s[2] * inv;
  const double A[6] = {S[0] * inv - cx * cx, S[1] * inv - cx * cy, S[2] * inv - cx * cz,
                       S[3] * inv - cy * cy, S[4] * inv - cy * cz, S[5] * inv - cz * cz};
  ag_plane_normal(A, nrm);
  ubar[0] = cx; ubar[1] = cy; ubar[2] = cz;
  far = 0.0;
  for (int j = 0; j < m; ++j) {
    const int a = mem[j];
    const double ux = at(a, 0) - ox - cx, uy = at(a, 1) - oy - cy, uz = at(a, 2) - oz - cz;
    far = fmax(far, fabs(nrm[0] * ux + nrm[1] * uy + nrm[2] * uz));
  }
  return true;
}

// one wave per conformer, lanes over the groups (strided past 64), shaped like k_pair_bounds; the plane of a lane's group comes
// from ag_group_plane.  All in fp64 from the fp32 coordinates; dev = the largest |projection| as fp32, +inf when a member
// coordinate is not finite.  A group of fewer than 3 or more than AGDIFF_PLANAR_MAX_ATOMS members, or one that names an atom
// outside [0, n), has dev = NaN, reads no coordinate and enters neither the maximum nor the count.
__global__ void __launch_bounds__(64) k_planar_groups(const float* __restrict__ pos, const int32_t* __restrict__ grp_ptr,
                                                      const int32_t* __restrict__ grp_idx, int n, int P, float thresh,
                                                      float* __restrict__ dev, float* __restrict__ worst,
                                                      int32_t* __restrict__ worst_group, int32_t* __restrict__ n_bent) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const float* p = pos + (size_t)g * n * 3;
  float best = -1.0f;                               // (below every deviation: the lane's first group is taken)
  int best_k = -1, bent = 0;
  for (int k = lane; k < P; k += 64) {
    const int b = grp_ptr[k], m = grp_ptr[k + 1] - b;
    bool ok = m >= 3 && m <= AGDIFF_PLANAR_MAX_ATOMS;
    for (int j = 0; ok && j < m; ++j) ok = ag_atoms_in_range(n, grp_idx[b + j]);
    float d = NAN;
    if (ok) {
      double org[3], ubar[3], nrm[3], far;
      const bool fin = ag_group_plane([p](int a, int c) { return (double)p[3 * a + c]; }, grp_idx + b, m, org, ubar, nrm, far);
      d = fin ? (float)far : INFINITY;
    }
    if (dev) dev[(size_t)g * P + k] = d;
    if (d == d) {                                   // (a NaN group takes no part)
      bent += d > thresh ? 1 : 0;
      if (d > best) { best = d; best_k = k; }       // (k ascends: the lane keeps its lowest k)
    }
  }
  ag_wave_worst(best, best_k, bent);
  if (lane == 0) {
    worst[g] = best_k < 0 ? 0.0f : best;
    worst_group[g] = best_k;
    n_bent[g] = bent;
  }
}

// (ratio, i, j) a is the better clash candidate than b: the smaller ratio, then the lowest i (j is already the lowest of its i);
// "no pair" carries i = INT32_MAX and loses to every pair, one of ratio +inf included
__device__ __forceinline__ bool ag_clash_better(float ra, int ia, float rb, int ib) { return ra < rb || (ra == rb && ia < ib); }

// Grid (S, G): a workgroup owns the atoms i of one slice of AGDIFF_CLASH_SLICE atoms of one conformer, thread t one i.  The
// atoms j are walked in tiles of the same size staged in LDS as (x, y, z, radius); every lane reads the same j (a broadcast),
// and only the tiles from the slice's own on are visited (j > i).  Each lane carries a cursor into its own ascending
// exclusion row: `nx`, the next excluded j, sits in a register and the row is read again only when j reaches it -- a two-pointer
// merge, O(n + degree) per atom, no n x n mask.
//   ratio = (float)(d / (r_i + r_j)) in fp64, 0 when d is not finite.
// Most pairs are far apart: a pair with d^2 > (c (r_i + r_j))^2 (1 + 1e-6), c = max(thresh, the lane's minimum so far), has a
// ratio above c after rounding too (fp32 rounding is monotonic and 1e-6 covers the fp64 error many times over), so it neither
// counts nor lowers the minimum and skips the square root and the division.
// One partial per (g, slice) goes to scratch: { bits(min ratio), i, j, count }, i = j = -1 when the slice has no pair.
__global__ void __launch_bounds__(AGDIFF_CLASH_SLICE) k_clash_scan(const float* __restrict__ pos, const float* __restrict__ radius,
                                                                   const int32_t* __restrict__ ex_ptr,
                                                                   const int32_t* __restrict__ ex_idx, int n, float thresh,
                                                                   int32_t* __restrict__ scratch) {
  __shared__ float4 s_atom[AGDIFF_CLASH_SLICE];
  __shared__ float s_r[AGDIFF_CLASH_SLICE / 64];
  __shared__ int32_t s_i[AGDIFF_CLASH_SLICE / 64], s_j[AGDIFF_CLASH_SLICE / 64], s_c[AGDIFF_CLASH_SLICE / 64];
  const int slice = blockIdx.x, g = blockIdx.y, S = gridDim.x, t = threadIdx.x;
  const float* p = pos + (size_t)g * n * 3;
  const int i = slice * AGDIFF_CLASH_SLICE + t;
  const bool active = i < n;
  double xi = 0.0, yi = 0.0, zi = 0.0, ri = 0.0;
  int cur = 0, end = 0;
  if (active) {
    xi = p[3 * i]; yi = p[3 * i + 1]; zi = p[3 * i + 2]; ri = radius[i];
    int lo_ = ex_ptr[i];
    end = ex_ptr[i + 1];
    int hi_ = end;
    while (lo_ < hi_) {                             // the first entry of the row above i
      const int mid = (lo_ + hi_) >> 1;
      if (ex_idx[mid] <= i) lo_ = mid + 1; else hi_ = mid;
    }
    cur = lo_;
  }
  int nx = cur < end ? ex_idx[cur] : 0x7fffffff;
  float minr = INFINITY;
  int minj = -1, count = 0;
  const double th = (double)thresh;
  double c2 = (double)INFINITY;                     // (max(thresh, minr))^2 (1 + 1e-6)
  for (int jt = slice; jt < S; ++jt) {
    const int j0 = jt * AGDIFF_CLASH_SLICE;
    __syncthreads();
    if (j0 + t < n) s_atom[t] = make_float4(p[3 * (j0 + t)], p[3 * (j0 + t) + 1], p[3 * (j0 + t) + 2], radius[j0 + t]);
    __syncthreads();
    const int cnt = min(AGDIFF_CLASH_SLICE, n - j0);
    if (!active) continue;
    for (int jj = 0; jj < cnt; ++jj) {
      const int j = j0 + jj;
      if (j <= i) continue;
      if (j == nx) {
        ++cur;
        nx = cur < end ? ex_idx[cur] : 0x7fffffff;
        continue;
      }
      const float4 q = s_atom[jj];
      const double dx = xi - (double)q.x, dy = yi - (double)q.y, dz = zi - (double)q.z;
      const double d2 = dx * dx + dy * dy + dz * dz, rs = ri + (double)q.w;
      if (d2 > c2 * (rs * rs) && d2 <= 1.79769313486231570e308) continue;
      const double d = sqrt(d2);
      const float r = d <= 1.79769313486231570e308 ? (float)(d / rs) : 0.0f;
      count += r < thresh ? 1 : 0;
      if (r < minr || minj < 0) {
        minr = r; minj = j;
        const double c = fmax(th, (double)r);
        c2 = c * c * (1.0 + 1e-6);
      }
    }
  }
  // the workgroup's (min, pair, count): across each wave by shuffles, then the four waves in order
  int mini = minj >= 0 ? i : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float orr = __shfl_xor(minr, o);
    const int oi = __shfl_xor(mini, o), oj = __shfl_xor(minj, o);
    count += __shfl_xor(count, o);
    if (ag_clash_better(orr, oi, minr, mini)) { minr = orr; mini = oi; minj = oj; }
  }
  if ((t & 63) == 0) { s_r[t >> 6] = minr; s_i[t >> 6] = mini; s_j[t >> 6] = minj; s_c[t >> 6] = count; }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < AGDIFF_CLASH_SLICE / 64; ++w) {
      count += s_c[w];
      if (ag_clash_better(s_r[w], s_i[w], minr, mini)) { minr = s_r[w]; mini = s_i[w]; minj = s_j[w]; }
    }
    int32_t* o = scratch + ((size_t)g * S + slice) * 4;
    o[0] = __float_as_int(minr);
    o[1] = minj >= 0 ? mini : -1;
    o[2] = minj;
    o[3] = count;
  }
}

// one wave per conformer: the S partials of k_clash_scan, lanes over the slices (strided past 64) in slice order
__global__ void __launch_bounds__(64) k_clash_finish(const int32_t* __restrict__ scratch, int S, float* __restrict__ min_ratio,
                                                     int32_t* __restrict__ min_pair, int32_t* __restrict__ n_clash) {
  const int g = blockIdx.x, lane = threadIdx.x;
  float minr = INFINITY;
  int mini = 0x7fffffff, minj = -1, count = 0;
  for (int s = lane; s < S; s += 64) {
    const int32_t* o = scratch + ((size_t)g * S + s) * 4;
    const float r = __int_as_float(o[0]);
    const int oi = o[1] >= 0 ? o[1] : 0x7fffffff;
    count += o[3];
    if (ag_clash_better(r, oi, minr, mini)) { minr = r; mini = oi; minj = o[2]; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float orr = __shfl_xor(minr, o);
    const int oi = __shfl_xor(mini, o), oj = __shfl_xor(minj, o);
    count += __shfl_xor(count, o);
    if (ag_clash_better(orr, oi, minr, mini)) { minr = orr; mini = oi; minj = oj; }
  }
  if (lane == 0) {
    min_ratio[g] = minr;
    min_pair[2 * g] = minj >= 0 ? mini : -1;
    min_pair[2 * g + 1] = minj;
    n_clash[g] = count;
  }
}

// ---- geometry repair: the atoms of a conformer that fails the two checks above moved into its distance bounds (not MMFF: no
// energies, no torsions, no electrostatics; include/agdiff_hip.h has the rule) --

#define AG_RELAX_THREADS 256

// (or of the flags, max of r) over the workgroup, in every thread: the xor butterfly in each wave, the four waves by thread 0 into
// ONE LDS value each, which every thread reads after the second barrier -- what a uniform loop exit needs.  The barriers also
// publish whatever the threads wrote to LDS before the call.
__device__ __forceinline__ void ag_relax_reduce(int& flags, double& r, int* s_wf, double* s_wr, int* s_flags, double* s_r) {
  const int t = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    flags |= __shfl_xor(flags, o);
    r = fmax(r, __shfl_xor(r, o));
  }
  if ((t & 63) == 0) { s_wf[t >> 6] = flags; s_wr[t >> 6] = r; }
  __syncthreads();
  if (t == 0) {
    int f = s_wf[0];
    double m = s_wr[0];
#pragma unroll
    for (int w = 1; w < AG_RELAX_THREADS / 64; ++w) { f |= s_wf[w]; m = fmax(m, s_wr[w]); }
    *s_flags = f;
    *s_r = m;
  }
  __syncthreads();
  flags = *s_flags;
  r = *s_r;
}

// a += h u, u the unit vector of (dx, dy, dz) of length d; atoms closer than 1e-9 part along x, the lower index towards +x
__device__ __forceinline__ void ag_relax_add(double& ax, double& ay, double& az, double h, double dx, double dy, double dz, double d,
                                             bool lower) {
  if (d < 1e-9) {
    ax += lower ? h : -h;
  } else {
    const double q = h / d;
    ax += q * dx; ay += q * dy; az += q * dz;
  }
}

// One workgroup per conformer, positions in LDS as fp64 in two buffers (a Jacobi update: every move is computed from the old
// positions), kCap atoms of room.  Atom i belongs to L consecutive lanes (L a power of two <= 64 with n L <= 256, so a group never
// leaves its wave; L = 1 past 128 atoms, atoms then strided over the threads): lane `sub` of the group takes the entries
// sub, sub + L, ... of the atom's bounded row and then the atoms j = sub, sub + L, ... -- every group of a wave reads the same L
// LDS addresses, a broadcast -- merging the atom's ascending exclusion row as j ascends, as k_clash_scan does; the L partial sums
// meet in the xor butterfly, offsets L / 2 ... 1.  The first pass also tests the conformer against the true bounds with the rules
// of k_pair_bounds and k_clash_scan.  A pair with d^2 > T^2 (1 + 1e-6) has c = 0 and, as T >= clash (r_i + r_j), a ratio that is
// not below `clash` after rounding either: it skips the square root.  Flags: 1 the stop rule is not met, 2 not valid at entry,
// 4 a coordinate that is not finite.
//
// kPlanes (k_relax_planar; without it every plane line below is compiled out and this is k_relax_bounds as it was): each iteration
// gets a phase A before the atom loop, thread k < P over group k: ag_group_plane on the current positions, the unit normal and
// the centroid to LDS as six doubles, structure of arrays (consecutive threads write consecutive doubles: no bank conflict), and on
// the first pass k_planar_groups' own verdict (float)dev > thresh into flag 2.  After a barrier the atom loop adds, for the groups
// of the atom's membership row mb_grp[mb_ptr[i] .. mb_ptr[i + 1]) (lane `sub` takes sub, sub + L, ...: a fixed order), the whole
// step -sign(h) e n onto the plane's target slab, h = n . (x_i - c), e = max(|h| - flat_to, 0), and the weight's denominator grows
// by the row's length q_i.  The next phase A overwrites the planes only after the two barriers of the reduction.
struct ag_planes_t {
  const int32_t *grp_ptr, *grp_idx, *mb_ptr, *mb_grp;
  int P;
  float thresh, flat_to;
};

template <int kCap, bool kPlanes>
__device__ __forceinline__ void ag_relax(const float* __restrict__ pos, const int32_t* __restrict__ bd_ptr,
                                         const int32_t* __restrict__ bd_idx, const float* __restrict__ bd_lo,
                                         const float* __restrict__ bd_hi, const float* __restrict__ radius,
                                         const int32_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_idx, int n, int L, float clash,
                                         float pad, float omega, int max_iter, const ag_planes_t& pl, float* __restrict__ pos_out,
                                         int32_t* __restrict__ status, int32_t* __restrict__ iters, float* __restrict__ resid,
                                         float* __restrict__ moved) {
  __shared__ double s_x[2][3][kCap];
  __shared__ float s_rad[kCap];
  __shared__ double s_pl[kPlanes ? 6 : 1][kPlanes ? AGDIFF_FLATTEN_MAX_GROUPS : 1];   // (not referenced without kPlanes: no LDS)
  __shared__ double s_wr[AG_RELAX_THREADS / 64], s_r;
  __shared__ int s_wf[AG_RELAX_THREADS / 64], s_flags;
  const int g = blockIdx.x, t = threadIdx.x;
  const float* p = pos + (size_t)g * n * 3;
  float* po = pos_out + (size_t)g * n * 3;
  int flags = 0;
  double rmax = 0.0;
  for (int a = t; a < n; a += AG_RELAX_THREADS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = p[3 * a + c];
      s_x[0][c][a] = v;
      flags |= ag_finite(v) ? 0 : 4;
    }
    s_rad[a] = radius[a];
  }
  ag_relax_reduce(flags, rmax, s_wf, s_wr, &s_flags, &s_r);
  if (flags) {                                      // not finite: copied through, bit for bit
    for (int e = t; e < 3 * n; e += AG_RELAX_THREADS) po[e] = p[e];
    if (t == 0) { status[g] = 3; iters[g] = 0; resid[g] = INFINITY; moved[g] = 0.0f; }
    return;
  }
  const int sub = t & (L - 1), slot = t / L, slots = AG_RELAX_THREADS / L;
  const double cl = (double)clash, pd = (double)pad, om = (double)omega;
  int cur = 0, it = 0, st = 0;
  bool first = true;
  for (;;) {
    const double(*x)[kCap] = s_x[cur];
    double(*y)[kCap] = s_x[cur ^ 1];
    flags = 0;
    rmax = 0.0;
    if constexpr (kPlanes) {                        // phase A: the plane of group t from the current positions
      if (t < pl.P) {
        const int b = pl.grp_ptr[t];
        double org[3], ubar[3], nrm[3] = {0.0, 0.0, 0.0}, far = 0.0;
        const bool fin = ag_group_plane([x](int a, int c) { return x[c][a]; }, pl.grp_idx + b, pl.grp_ptr[t + 1] - b, org, ubar, nrm, far);
        if (first && (float)far > pl.thresh) flags |= 2;
#pragma unroll
        for (int c = 0; c < 3; ++c) {               // (positions that left the finite range: a zero normal, the group moves nothing)
          s_pl[c][t] = fin ? nrm[c] : 0.0;
          s_pl[3 + c][t] = fin ? org[c] + ubar[c] : 0.0;
        }
      }
      __syncthreads();
    }
    for (int i = slot; i < n; i += slots) {         // (L > 1: n <= slots, one turn, whole groups in or out)
      const double xi = x[0][i], yi = x[1][i], zi = x[2][i], ri = (double)s_rad[i];
      double ax = 0.0, ay = 0.0, az = 0.0;
      const int b0 = bd_ptr[i], b1 = bd_ptr[i + 1];
      for (int k = b0 + sub; k < b1; k += L) {
        const int j = bd_idx[k];
        const double lo = (double)bd_lo[k], hi = (double)bd_hi[k];
        const double dx = xi - x[0][j], dy = yi - x[1][j], dz = zi - x[2][j];
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        if (first) {
          const double df = (double)(float)d;
          if ((float)fmax(fmax(lo - df, df - hi), 0.0) > 0.0f) flags |= 2;
        }
        const double pk = fmin(pd, 0.5 * (hi - lo));
        double s = 0.0;
        if (d < lo + pk) s = lo + pk - d;
        else if (d > hi - pk) s = hi - pk - d;
        if (fabs(s) > 0.5 * pk) flags |= 1;
        rmax = fmax(rmax, fabs(s));
        if (s != 0.0) ag_relax_add(ax, ay, az, 0.5 * s, dx, dy, dz, d, i < j);
      }
      int c = ex_ptr[i];
      const int e = ex_ptr[i + 1];
      int nx = c < e ? ex_idx[c] : 0x7fffffff;
      for (int j = sub; j < n; j += L) {
        while (nx < j) {
          ++c;
          nx = c < e ? ex_idx[c] : 0x7fffffff;
        }
        if (j == i || j == nx) continue;
        const double rs = ri + (double)s_rad[j], T = cl * rs + pd;
        const double dx = xi - x[0][j], dy = yi - x[1][j], dz = zi - x[2][j];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 > T * T * (1.0 + 1e-6)) continue;
        const double d = sqrt(d2);
        if (first && (float)(d / rs) < clash) flags |= 2;
        const double cc = fmax(T - d, 0.0);
        if (cc > 0.5 * pd) flags |= 1;
        rmax = fmax(rmax, cc);
        if (cc > 0.0) ag_relax_add(ax, ay, az, 0.5 * cc, dx, dy, dz, d, i < j);
      }
      int q = 0;
      if constexpr (kPlanes) {
        const int m0 = pl.mb_ptr[i], m1 = pl.mb_ptr[i + 1];
        q = m1 - m0;
        const double ft = (double)pl.flat_to;
        for (int k = m0 + sub; k < m1; k += L) {
          const int gk = pl.mb_grp[k];
          const double nx_ = s_pl[0][gk], ny_ = s_pl[1][gk], nz_ = s_pl[2][gk];
          const double h = nx_ * (xi - s_pl[3][gk]) + ny_ * (yi - s_pl[4][gk]) + nz_ * (zi - s_pl[5][gk]);
          const double ee = fmax(fabs(h) - ft, 0.0);
          if (ee > 0.5 * pd) flags |= 1;
          rmax = fmax(rmax, ee);
          if (ee > 0.0) {
            const double mv = h > 0.0 ? -ee : ee;
            ax += mv * nx_; ay += mv * ny_; az += mv * nz_;
          }
        }
      }
      for (int o = L >> 1; o > 0; o >>= 1) {
        ax += __shfl_xor(ax, o); ay += __shfl_xor(ay, o); az += __shfl_xor(az, o);
      }
      if (sub == 0) {
        const double w = om / (double)(b1 - b0 + q + 1);
        y[0][i] = xi + w * ax; y[1][i] = yi + w * ay; y[2][i] = zi + w * az;
      }
    }
    ag_relax_reduce(flags, rmax, s_wf, s_wr, &s_flags, &s_r);
    if (first) {
      first = false;
      if (!(flags & 2)) { st = 0; break; }
    }
    if (!(flags & 1)) { st = 1; break; }
    if (it == max_iter) { st = 2; break; }
    cur ^= 1;                                       // the displacements are applied
    ++it;
  }
  if (st == 0) {                                    // valid as it came: copied through, bit for bit
    for (int e = t; e < 3 * n; e += AG_RELAX_THREADS) po[e] = p[e];
    if (t == 0) { status[g] = 0; iters[g] = 0; resid[g] = 0.0f; moved[g] = 0.0f; }
    return;
  }
  const double resid_out = rmax;
  double m2 = 0.0;
  for (int a = t; a < n; a += AG_RELAX_THREADS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = s_x[cur][c][a], dv = v - (double)p[3 * a + c];
      m2 += dv * dv;
      po[3 * a + c] = (float)v;
    }
  }
  ag_wave_sum(m2);
  if ((t & 63) == 0) s_wr[t >> 6] = m2;             // (s_wr: last read before the second barrier of the last reduction)
  __syncthreads();
  if (t == 0) {
    m2 = 0.0;
#pragma unroll
    for (int w = 0; w < AG_RELAX_THREADS / 64; ++w) m2 += s_wr[w];
    status[g] = st;
    iters[g] = it;
    resid[g] = (float)resid_out;
    moved[g] = (float)sqrt(m2 / n);
  }
}

template <int kCap>
__global__ void __launch_bounds__(AG_RELAX_THREADS) k_relax_bounds(const float* __restrict__ pos, const int32_t* __restrict__ bd_ptr,
                                                                   const int32_t* __restrict__ bd_idx, const float* __restrict__ bd_lo,
                                                                   const float* __restrict__ bd_hi, const float* __restrict__ radius,
                                                                   const int32_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_idx,
                                                                   int n, int L, float clash, float pad, float omega, int max_iter,
                                                                   float* __restrict__ pos_out, int32_t* __restrict__ status,
                                                                   int32_t* __restrict__ iters, float* __restrict__ resid,
                                                                   float* __restrict__ moved) {
  ag_relax<kCap, false>(pos, bd_ptr, bd_idx, bd_lo, bd_hi, radius, ex_ptr, ex_idx, n, L, clash, pad, omega, max_iter, ag_planes_t{},
                        pos_out, status, iters, resid, moved);
}

// k_relax_bounds plus the planes of P <= AGDIFF_FLATTEN_MAX_GROUPS groups (one group per thread in phase A); P = 0 gives
// k_relax_bounds' results
template <int kCap>
__global__ void __launch_bounds__(AG_RELAX_THREADS) k_relax_planar(const float* __restrict__ pos, const int32_t* __restrict__ bd_ptr,
                                                                   const int32_t* __restrict__ bd_idx, const float* __restrict__ bd_lo,
                                                                   const float* __restrict__ bd_hi, const float* __restrict__ radius,
                                                                   const int32_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_idx,
                                                                   int n, int L, float clash, float pad, float omega, int max_iter,
                                                                   ag_planes_t pl, float* __restrict__ pos_out,
                                                                   int32_t* __restrict__ status, int32_t* __restrict__ iters,
                                                                   float* __restrict__ resid, float* __restrict__ moved) {
  ag_relax<kCap, true>(pos, bd_ptr, bd_idx, bd_lo, bd_hi, radius, ex_ptr, ex_idx, n, L, clash, pad, omega, max_iter, pl, pos_out, status,
                       iters, resid, moved);
}

// ---- distance-distribution MMD (ConfGF / CGCF / GraphDG; include/agdiff_hip.h has the definition): Z = [X; Y], M = R + G rows of
// K interatomic distances.  "all" is one problem over the rows, "single" one problem per column.  Everything is fp64 from the
// stored fp32 values; every sum has a fixed order (thread-strided terms, the xor butterfly, then waves or tiles in index order).

// row a of Z = [X; Y]
__device__ __forceinline__ const float* ag_mmd_row(const float* __restrict__ x, const float* __restrict__ y, int R, int K, int a) {
  return a < R ? x + (size_t)a * K : y + (size_t)(a - R) * K;
}

// k = sum_{i = 0 .. 4} exp(-D2 / (b 2^(i - 2))) from ninv = -1 / (4 b): ONE exponential, of the widest bandwidth, and four
// squarings (e^2, e^4, e^8, e^16 are the bandwidths 2 b, b, b / 2, b / 4).  D2 = 0 gives exactly 5.
__device__ __forceinline__ double ag_mmd_kernel(double d2, double ninv) {
  const double e1 = exp(d2 * ninv), e2 = e1 * e1, e4 = e2 * e2, e8 = e4 * e4, e16 = e8 * e8;
  return (((e16 + e8) + e4) + e2) + e1;
}

// pair a <= b of the upper triangle into the three ordered-pair sums: XX and YY count (a, b) and (b, a), the diagonal once; XY counts
// each reference-generated pair once
__device__ __forceinline__ void ag_mmd_add(int a, int b, int R, double v, double& xx, double& yy, double& xy) {
  const double w = a == b ? v : 2.0 * v;            // (selects, not branches: the lanes of a wave differ in their class)
  xx += b < R ? w : 0.0;
  yy += a >= R ? w : 0.0;
  xy += (a < R && b >= R) ? v : 0.0;
}

// mmd2 from the three sums; b == 0 (every row equal) is 0, a bandwidth that is not finite (a non-finite entry) NaN
__device__ __forceinline__ float ag_mmd_value(double xx, double yy, double xy, int R, int G, double b) {
  if (b == 0.0) return 0.0f;
  if (!ag_finite(b)) return __builtin_nanf("");
  return (float)((xx / ((double)R * R) + yy / ((double)G * G)) - 2.0 * (xy / ((double)R * G)));
}

// Statistics pass: per column c the scatter q[c] = sum_a (Z[a][c] - mu_c)^2 around the column mean (NaN when the column holds an
// entry that is not finite), from which b = 2 M q / (M^2 - M) is the mean of D2 over the ordered pairs a != b without a pass over
// pairs and without cancellation.  Workgroup = 16 columns; thread (ty, tx) walks the rows ty, ty + 16, ... of column c0 + tx (64-byte
// segments of a table row), the 16 stripes are summed through LDS in stripe order.  With zt it also writes the table transposed,
// zt [K][M], through a 16 x 17 LDS tile (64-byte segments again), so that k_mmd_single reads a column contiguously; with bw / bw32
// the per-column bandwidths.
__global__ void __launch_bounds__(256) k_mmd_stats(const float* __restrict__ x, const float* __restrict__ y, int R, int G, int K,
                                                   float* __restrict__ zt, double* __restrict__ scatter, double* __restrict__ bw,
                                                   float* __restrict__ bw32) {
  __shared__ float tile[16][17];
  __shared__ double red[16][16];
  __shared__ int redbad[16][16];
  const int M = R + G, c0 = blockIdx.x * 16;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const int c = c0 + tx;
  double s = 0.0;
  int bad = 0;
  for (int a0 = 0; a0 < M; a0 += 16) {
    const int a = a0 + ty;
    float z = 0.0f;
    if (a < M && c < K) {
      z = ag_mmd_row(x, y, R, K, a)[c];
      s += (double)z;
      bad |= !ag_finite((double)z);
    }
    if (zt) {                                       // (uniform: the barriers are reached by every thread)
      tile[ty][tx] = z;
      __syncthreads();
      if (c0 + ty < K && a0 + tx < M) zt[(size_t)(c0 + ty) * M + a0 + tx] = tile[tx][ty];
      __syncthreads();
    }
  }
  red[ty][tx] = s;
  redbad[ty][tx] = bad;
  __syncthreads();
  double sum = 0.0;
  bad = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) { sum += red[r][tx]; bad |= redbad[r][tx]; }
  const double mu = sum / (double)M;
  __syncthreads();
  double q = 0.0;
  if (c < K)
    for (int a = ty; a < M; a += 16) {
      const double d = (double)ag_mmd_row(x, y, R, K, a)[c] - mu;
      q += d * d;
    }
  red[ty][tx] = q;
  __syncthreads();
  if (ty == 0 && c < K) {
    double qs = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) qs += red[r][tx];
    if (bad) qs = __builtin_nan("");
    scatter[c] = qs;
    if (bw) {
      const double b = (2.0 * (double)M * qs) / ((double)M * (double)M - (double)M);
      bw[c] = b;
      bw32[c] = (float)b;
    }
  }
}

// one wave: the "all" bandwidth from the K column scatters, lanes striding over the columns
__global__ void __launch_bounds__(64) k_mmd_bandwidth(const double* __restrict__ scatter, int K, int M, double* __restrict__ bw,
                                                      float* __restrict__ bw32) {
  double q = 0.0;
  for (int c = threadIdx.x; c < K; c += 64) q += scatter[c];
  ag_wave_sum(q);
  if (threadIdx.x == 0) {
    const double b = (2.0 * (double)M * q) / ((double)M * (double)M - (double)M);
    *bw = b;
    *bw32 = (float)b;
  }
}

// "all": one workgroup per 16 x 16 tile of the upper triangle of the M x M row pairs, thread (ty, tx) = rows (i0 + ty, j0 + tx).  The
// 16 + 16 table rows are staged in LDS AG_MMD_CHUNK columns at a time at an odd pitch (the 16 tx of a tile row read 16 different
// banks, the ty row is a broadcast).  A diagonal tile counts ty <= tx only.  One partial { XX, YY, XY } per tile.
#define AG_MMD_CHUNK 64
__global__ void __launch_bounds__(256) k_mmd_all(const float* __restrict__ x, const float* __restrict__ y, int R, int G, int K, int T,
                                                 const double* __restrict__ bw, double* __restrict__ partial) {
  __shared__ float srow[16][AG_MMD_CHUNK + 1];
  __shared__ float scol[16][AG_MMD_CHUNK + 1];
  __shared__ double sred[4][3];
  const double b = *bw;
  if (!(b > 0.0)) return;                           // (uniform; k_mmd_all_finish does not read the partials then)
  const double ninv = -0.25 / b;
  const int M = R + G;
  int ti, tj;
  ag_triangle_tile((long long)blockIdx.x, T, ti, tj);
  const int i0 = ti * 16, j0 = tj * 16;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const int ai = i0 + ty, aj = j0 + tx;
  const bool valid = ai < M && aj < M && ai <= aj;
  double d2 = 0.0;
  for (int k0 = 0; k0 < K; k0 += AG_MMD_CHUNK) {
    const int kc = K - k0 < AG_MMD_CHUNK ? K - k0 : AG_MMD_CHUNK;
    for (int t = threadIdx.x; t < 16 * AG_MMD_CHUNK; t += 256) {
      const int r = t / AG_MMD_CHUNK, o = t % AG_MMD_CHUNK;
      srow[r][o] = (i0 + r < M && o < kc) ? ag_mmd_row(x, y, R, K, i0 + r)[k0 + o] : 0.0f;
      scol[r][o] = (j0 + r < M && o < kc) ? ag_mmd_row(x, y, R, K, j0 + r)[k0 + o] : 0.0f;
    }
    __syncthreads();
    if (valid)
      for (int o = 0; o < kc; ++o) {
        const double d = (double)srow[ty][o] - (double)scol[tx][o];
        d2 += d * d;
      }
    __syncthreads();
  }
  double xx = 0.0, yy = 0.0, xy = 0.0;
  if (valid) ag_mmd_add(ai, aj, R, ag_mmd_kernel(d2, ninv), xx, yy, xy);
  ag_wave_sum(xx, yy, xy);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sred[wave][0] = xx; sred[wave][1] = yy; sred[wave][2] = xy; }
  __syncthreads();
  const int e = threadIdx.x;
  if (e < 3) partial[(size_t)blockIdx.x * 3 + e] = ((sred[0][e] + sred[1][e]) + sred[2][e]) + sred[3][e];
}

// one wave: the tile partials, lanes striding over the tiles in tile order
__global__ void __launch_bounds__(64) k_mmd_all_finish(const double* __restrict__ partial, long long tiles, const double* __restrict__ bw,
                                                       int R, int G, float* __restrict__ mmd2) {
  const double b = *bw;
  double xx = 0.0, yy = 0.0, xy = 0.0;
  if (b > 0.0)
    for (long long t = threadIdx.x; t < tiles; t += 64) { xx += partial[3 * t]; yy += partial[3 * t + 1]; xy += partial[3 * t + 2]; }
  ag_wave_sum(xx, yy, xy);
  if (threadIdx.x == 0) *mmd2 = ag_mmd_value(xx, yy, xy, R, G, b);
}

// "single": one workgroup per column, its M values in LDS (read contiguously from the transposed table of k_mmd_stats).  The pairs
// a <= b are numbered row by row, p = 0 .. M (M + 1) / 2 - 1, and thread t takes p = t, t + 1024, ...: every thread the same number
// of pairs to within one, whatever M is; the lanes of a wave read consecutive b and (mostly) one a.  Thread sums, butterfly, then
// the 16 waves in wave order.
#define AG_MMD_SINGLE_THREADS 1024
__global__ void __launch_bounds__(AG_MMD_SINGLE_THREADS) k_mmd_single(const float* __restrict__ zt, const double* __restrict__ bw, int R,
                                                                      int G, float* __restrict__ mmd2) {
  __shared__ double sred[AG_MMD_SINGLE_THREADS / 64][3];
  float* z = ag_eval_smem;                          // [M]
  const int M = R + G, c = blockIdx.x;
  const double b = bw[c];
  if (!(b > 0.0)) {                                 // (uniform)
    if (threadIdx.x == 0) mmd2[c] = ag_mmd_value(0.0, 0.0, 0.0, R, G, b);
    return;
  }
  const double ninv = -0.25 / b;
  for (int a = threadIdx.x; a < M; a += AG_MMD_SINGLE_THREADS) z[a] = zt[(size_t)c * M + a];
  __syncthreads();
  double xx = 0.0, yy = 0.0, xy = 0.0;
  int a = 0, off = threadIdx.x;                     // pair (a, a + off); row a holds M - a pairs
  while (a < M && off >= M - a) { off -= M - a; ++a; }
  while (a < M) {
    const double d = (double)z[a] - (double)z[a + off];
    ag_mmd_add(a, a + off, R, ag_mmd_kernel(d * d, ninv), xx, yy, xy);
    off += AG_MMD_SINGLE_THREADS;
    while (a < M && off >= M - a) { off -= M - a; ++a; }
  }
  ag_wave_sum(xx, yy, xy);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sred[wave][0] = xx; sred[wave][1] = yy; sred[wave][2] = xy; }
  __syncthreads();
  if (threadIdx.x == 0) {
    xx = yy = xy = 0.0;
    for (int w = 0; w < AG_MMD_SINGLE_THREADS / 64; ++w) { xx += sred[w][0]; yy += sred[w][1]; xy += sred[w][2]; }
    mmd2[c] = ag_mmd_value(xx, yy, xy, R, G, b);
  }
}

}  // namespace

// bytes per row of a threshold bit-matrix of `columns` columns: 16-bit pieces, rounded up to 8 bytes
static int ag_bits_pitch(int columns) { return ((columns + 15) / 16 * 2 + 7) / 8 * 8; }

// The G == 0 answer of a walk, which launches nothing: every listed output set byte-wise (0: all bits clear; 0xff: NaNs) by
// memsets on the stream.  Without a device there is nothing to write to, and that is no error.
struct ag_fill { void* p; int byte; size_t bytes; };
static int ag_fill_outputs(std::initializer_list<ag_fill> outs, hipStream_t st) {
  for (const ag_fill& o : outs) {
    const hipError_t e = hipMemsetAsync(o.p, o.byte, o.bytes, st);
    if (e == hipSuccess) continue;
    (void)hipGetLastError();
    return e == hipErrorNoDevice ? AGDIFF_OK : AGDIFF_ERR_LAUNCH;
  }
  return AGDIFF_OK;
}

// the launch shape of a row pass with K bins per row (ag_row_pass<4> or <1>): one row per wave while the 4 K bins of a workgroup
// fit AG_ROW_BIN_BYTES, one row per workgroup above
struct ag_row_launch { bool wave_rows; dim3 grid; size_t lds; };
static ag_row_launch ag_row_pass_launch(int G, int K) {
  if (K <= AG_ROW_WAVE_MAX_K) return {true, dim3((unsigned)((G + 3) / 4)), (size_t)4 * K * 8};
  return {false, dim3((unsigned)G), (size_t)K * 8};
}

// agdiff_rmsd_matrix (out_mirror unused) and agdiff_rmsd_matrix_hands: the shared argument checks, both centring launches and
// the matrix kernel
template <bool kMirror>
static int ag_rmsd_matrix(const float* pos_ref, const float* pos_gen, const int32_t* atom_idx, const int32_t* perms, int32_t R,
                          int32_t G, int32_t n, int32_t m, int32_t P, float* scratch, float* out, float* out_mirror, void* stream) {
  if (!pos_ref || !pos_gen || !atom_idx || !scratch || !out || R < 0 || G < 0 || n <= 0 || m <= 0 || m > n || (perms && P <= 0))
    return AGDIFF_ERR_ARG;
  if (m > AGDIFF_RMSD_MAX_ATOMS) return AGDIFF_ERR_LIMIT;
  if (R == 0 || G == 0) return AGDIFF_OK;
  hipStream_t st = (hipStream_t)stream;
  float* cref = scratch;
  float* cgen = scratch + (size_t)R * (3 * m + 1);
  k_center_selected<<<dim3((unsigned)R), dim3(64), 0, st>>>(pos_ref, atom_idx, n, m, cref);
  AG_CHECK_LAUNCH();
  k_center_selected<<<dim3((unsigned)G), dim3(64), 0, st>>>(pos_gen, atom_idx, n, m, cgen);
  AG_CHECK_LAUNCH();
  const size_t smem = (size_t)2 * 16 * (3 * m + 1) * sizeof(float);
  static std::atomic<uint64_t> attr_done{0};        // (one per instantiation: ag_allow_big_lds records it per kernel function)
  if (smem > 48 * 1024 &&
      !ag_allow_big_lds(attr_done, (size_t)2 * 16 * (3 * AGDIFF_RMSD_MAX_ATOMS + 1) * sizeof(float), k_rmsd_matrix<kMirror>))
    return AGDIFF_ERR_LAUNCH;
  k_rmsd_matrix<kMirror><<<dim3((unsigned)((G + 15) / 16), (unsigned)((R + 15) / 16)), dim3(256), smem, st>>>(cref, cgen, perms, R, G, m, P,
                                                                                                            out, out_mirror);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_rmsd_matrix(const float* pos_ref, const float* pos_gen, const int32_t* atom_idx, const int32_t* perms,
                                  int32_t R, int32_t G, int32_t n, int32_t m, int32_t P, float* scratch, float* out,
                                  void* stream) {
  return ag_rmsd_matrix<false>(pos_ref, pos_gen, atom_idx, perms, R, G, n, m, P, scratch, out, nullptr, stream);
}

extern "C" int agdiff_matrix_minima(const float* mat, int32_t R, int32_t G, float* row_min, float* col_min, void* stream) {
  if (!mat || !row_min || !col_min || R <= 0 || G <= 0) return AGDIFF_ERR_ARG;
  const int mx = R > G ? R : G;
  k_matrix_minima<<<dim3((unsigned)mx, 2), dim3(64), 0, (hipStream_t)stream>>>(mat, R, G, row_min, col_min);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_rmsd_self(const float* pos, const int32_t* atom_idx, const int32_t* perms, int32_t G, int32_t n, int32_t m,
                                int32_t P, float thresh, float* scratch, float* out, uint64_t* bits, void* stream) {
  if (!pos || !atom_idx || !scratch || (!out && !bits) || G < 0 || n <= 0 || m <= 0 || m > n || (perms && P <= 0)) return AGDIFF_ERR_ARG;
  if (bits && (!(thresh >= 0.0f) || ((uintptr_t)bits & 7))) return AGDIFF_ERR_ARG;
  if (m > AGDIFF_RMSD_MAX_ATOMS) return AGDIFF_ERR_LIMIT;
  if (G == 0) return AGDIFF_OK;
  hipStream_t st = (hipStream_t)stream;
  k_center_selected<<<dim3((unsigned)G), dim3(64), 0, st>>>(pos, atom_idx, n, m, scratch);
  AG_CHECK_LAUNCH();
  const int64_t T = ((int64_t)G + 15) / 16;
  const int64_t tiles = T * (T + 1) / 2;
  if (tiles > 0x7fffffffll) return AGDIFF_ERR_LIMIT;
  const auto smem_for = [](int mm) { return ((size_t)2 * 16 * (3 * mm + 1) + 2 * 16 * 17) * sizeof(float); };
  static std::atomic<uint64_t> attr_done{0};
  if (smem_for(m) > 48 * 1024 && !ag_allow_big_lds(attr_done, smem_for(AGDIFF_RMSD_MAX_ATOMS), k_rmsd_self)) return AGDIFF_ERR_LAUNCH;
  k_rmsd_self<<<dim3((unsigned)tiles), dim3(256), smem_for(m), st>>>(scratch, perms, G, m, P, (int)T, thresh, out, (uint16_t*)bits,
                                                                           ag_bits_pitch(G));
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_leader_prune(const uint64_t* bits, int32_t G, int32_t* keep, int32_t* leader, int32_t* count, int32_t* n_kept,
                                   void* stream) {
  if (!bits || !keep || !leader || !count || !n_kept || G < 0 || ((uintptr_t)bits & 7)) return AGDIFF_ERR_ARG;
  if (G > AGDIFF_PRUNE_MAX_CONFS) return AGDIFF_ERR_LIMIT;
  const int words = ag_bits_pitch(G) / 8;                 // 64-bit words per row
  k_leader_prune<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(bits, G, words, keep, leader, count, n_kept);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_butina_cluster(const uint64_t* bits, int32_t G, int32_t reorder, int32_t* leader, int32_t* count, int32_t* rank,
                                     int32_t* n_clusters, void* stream) {
  if (!bits || !leader || !count || !rank || !n_clusters || G < 0 || (reorder != 0 && reorder != 1) || ((uintptr_t)bits & 7))
    return AGDIFF_ERR_ARG;
  if (G > AGDIFF_PRUNE_MAX_CONFS) return AGDIFF_ERR_LIMIT;
  if (G == 0) return ag_fill_outputs({{n_clusters, 0, 4}}, (hipStream_t)stream);      // no launch: n_clusters = 0
  const int words = ag_bits_pitch(G) / 8;                 // 64-bit words per row
  k_butina_cluster<<<dim3(1), dim3(AG_BUTINA_THREADS), 0, (hipStream_t)stream>>>(bits, G, words, reorder, leader, count, rank, n_clusters);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_maxmin_pick(const float* dist, int32_t G, int32_t K, int32_t first, float stop, int32_t* picks, float* radius,
                                  int32_t* owner, float* near, int32_t* n_picked, float* cover, void* stream) {
  if (!dist || !picks || !radius || !owner || !near || !n_picked || !cover || G < 0) return AGDIFF_ERR_ARG;
  if (G > 0 && (K < 1 || K > G || first < 0 || first >= G || stop != stop)) return AGDIFF_ERR_ARG;
  if (G > AGDIFF_PRUNE_MAX_CONFS) return AGDIFF_ERR_LIMIT;
  if (G == 0) return ag_fill_outputs({{n_picked, 0, 4}, {cover, 0, 4}}, (hipStream_t)stream);      // no launch: n_picked = 0, cover = 0
  k_maxmin_pick<<<dim3(1), dim3(AG_MAXMIN_THREADS), 0, (hipStream_t)stream>>>(dist, G, K, first, stop, picks, radius, owner, near, n_picked,
                                                                            cover);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

// the argument checks and the G == 0 answer that agdiff_kmedoids, agdiff_pam_build and agdiff_pam_swap share (`rest_ok`: the
// caller's own conditions, which count with K's when G > 0; n_steps: n_iter or n_swaps); returns AGDIFF_OK with *launch = false
// when there is nothing to launch
static int ag_kmed_prepare(const float* dist, int32_t G, int32_t K, bool rest_ok, int32_t* medoids, int32_t* labels, float* near,
                           int32_t* size, double* within, double* cost, int32_t* n_steps, int32_t* status, uint64_t* work,
                           hipStream_t st, bool* launch) {
  *launch = false;
  if (!dist || !medoids || !labels || !near || !size || !within || !cost || !n_steps || !status || !work || G < 0) return AGDIFF_ERR_ARG;
  if (G > 0 && (K < 1 || K > G || !rest_ok)) return AGDIFF_ERR_ARG;
  if ((uintptr_t)work & 7) return AGDIFF_ERR_ARG;
  if (G > AGDIFF_PRUNE_MAX_CONFS) return AGDIFF_ERR_LIMIT;
  if (G == 0) return ag_fill_outputs({{n_steps, 0, 4}, {status, 0, 4}, {cost, 0, 8}}, st);      // n_steps = 0, status = 0, cost = 0
  *launch = true;
  return AGDIFF_OK;
}

extern "C" int agdiff_kmedoids(const float* dist, int32_t G, int32_t K, const int32_t* init, int32_t max_iter, int32_t* medoids,
                               int32_t* labels, float* near, int32_t* size, double* within, double* cost, int32_t* n_iter,
                               int32_t* status, uint64_t* work, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  bool launch;
  if (!init) return AGDIFF_ERR_ARG;
  const int rc = ag_kmed_prepare(dist, G, K, max_iter >= 1 && max_iter <= AGDIFF_KMEDOIDS_MAX_ITER, medoids, labels, near, size, within,
                                 cost, n_iter, status, work, st, &launch);
  if (!launch) return rc;
  int32_t* ctl = (int32_t*)work;
  uint64_t* keys = work + KM_CTL_WORDS * 4 / 8;
  const dim3 cols((unsigned)((G + 63) / 64)), rows((unsigned)((G + 3) / 4));
  k_kmed_init<<<dim3(1), dim3(1024), 0, st>>>(dist, G, K, init, medoids, labels, near, size, within, cost, n_iter, status, ctl);
  AG_CHECK_LAUNCH();
  for (int it = 0; it < max_iter; ++it) {           // every launch returns at once after the update that ended the walk
    k_kmed_assign<<<cols, dim3(256), 0, st>>>(dist, G, K, init, medoids, labels, near, ctl, 0);
    AG_CHECK_LAUNCH();
    k_kmed_costs<<<rows, dim3(256), 0, st>>>(dist, G, labels, keys, ctl);
    AG_CHECK_LAUNCH();
    k_kmed_choose<<<dim3(1), dim3(1024), 0, st>>>(G, K, max_iter, labels, keys, medoids, ctl);
    AG_CHECK_LAUNCH();
  }
  k_kmed_assign<<<cols, dim3(256), 0, st>>>(dist, G, K, init, medoids, labels, near, ctl, 1);
  AG_CHECK_LAUNCH();
  k_kmed_finish<<<dim3(1), dim3(1024), 0, st>>>(G, K, labels, near, size, within, cost, n_iter, status, ctl);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

// agdiff_pam_build's and agdiff_pam_swap's carving of `work`
struct ag_pam_work {
  int32_t* ctl; uint64_t *dn, *ds; int64_t* recD; int32_t *tag, *recR;
  explicit ag_pam_work(uint64_t* work)
      : ctl((int32_t*)work), dn(work + KM_CTL_WORDS * 4 / 8), ds(dn + AGDIFF_PRUNE_MAX_CONFS),
        recD((int64_t*)(ds + AGDIFF_PRUNE_MAX_CONFS)), tag((int32_t*)(recD + AGDIFF_PRUNE_MAX_CONFS)),
        recR(tag + AGDIFF_PRUNE_MAX_CONFS) {}
};

extern "C" int agdiff_pam_build(const float* dist, int32_t G, int32_t K, int32_t anchor, int32_t* medoids, int32_t* labels, float* near,
                                int32_t* size, double* within, double* cost, int32_t* n_swaps, int32_t* status, uint64_t* work,
                                void* stream) {
  hipStream_t st = (hipStream_t)stream;
  bool launch;
  const int rc = ag_kmed_prepare(dist, G, K, true, medoids, labels, near, size, within, cost, n_swaps, status, work, st, &launch);
  if (!launch) return rc;
  const ag_pam_work w(work);
  const dim3 cols((unsigned)((G + 63) / 64)), rows((unsigned)((G + 3) / 4));
  k_pam_build_init<<<dim3(1), dim3(1024), 0, st>>>(dist, G, K, anchor, medoids, labels, near, size, within, cost, n_swaps, status, w.ctl,
                                                   w.dn, w.tag);
  AG_CHECK_LAUNCH();
  for (int p = 0; p < K; ++p) {                     // one pass over the candidates' rows and one pick per rank
    k_pam_rows<4, false><<<rows, dim3(256), 0, st>>>(dist, G, K, w.tag, w.dn, w.ds, w.recD, w.recR, w.ctl);
    AG_CHECK_LAUNCH();
    k_pam_build_pick<<<dim3(1), dim3(1024), 0, st>>>(dist, G, p, w.recD, medoids, w.dn, w.tag, w.ctl);
    AG_CHECK_LAUNCH();
  }
  k_pam_state<<<cols, dim3(256), 0, st>>>(dist, G, K, anchor, medoids, labels, near, w.ctl, w.dn, w.ds, w.tag, 0);
  AG_CHECK_LAUNCH();
  k_kmed_finish<<<dim3(1), dim3(1024), 0, st>>>(G, K, labels, near, size, within, cost, n_swaps, status, w.ctl);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_pam_swap(const float* dist, int32_t G, int32_t K, const int32_t* init, int32_t anchor, int32_t max_swaps,
                               int32_t* medoids, int32_t* labels, float* near, int32_t* size, double* within, double* cost,
                               int32_t* n_swaps, int32_t* status, uint64_t* work, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  bool launch;
  if (!init) return AGDIFF_ERR_ARG;
  const int rc = ag_kmed_prepare(dist, G, K, max_swaps >= 0 && max_swaps <= AGDIFF_PAM_MAX_SWAPS, medoids, labels, near, size, within,
                                 cost, n_swaps, status, work, st, &launch);
  if (!launch) return rc;
  const ag_pam_work w(work);
  const dim3 cols((unsigned)((G + 63) / 64));
  const ag_row_launch rows = ag_row_pass_launch(G, K);
  const auto k_rows = rows.wave_rows ? k_pam_rows<4, true> : k_pam_rows<1, true>;
  k_pam_swap_init<<<dim3(1), dim3(1024), 0, st>>>(dist, G, K, init, anchor, medoids, labels, near, size, within, cost, n_swaps, status,
                                                  w.ctl);
  AG_CHECK_LAUNCH();
  for (int it = 0; it < max_swaps; ++it) {          // every launch returns at once after the choose that ended the walk
    k_pam_state<<<cols, dim3(256), 0, st>>>(dist, G, K, anchor, medoids, labels, near, w.ctl, w.dn, w.ds, w.tag, 0);
    AG_CHECK_LAUNCH();
    k_rows<<<rows.grid, dim3(256), rows.lds, st>>>(dist, G, K, w.tag, w.dn, w.ds, w.recD, w.recR, w.ctl);
    AG_CHECK_LAUNCH();
    k_pam_choose<<<dim3(1), dim3(1024), 0, st>>>(G, max_swaps, w.recD, w.recR, medoids, w.ctl);
    AG_CHECK_LAUNCH();
  }
  k_pam_state<<<cols, dim3(256), 0, st>>>(dist, G, K, anchor, medoids, labels, near, w.ctl, w.dn, w.ds, w.tag, 1);
  AG_CHECK_LAUNCH();
  k_kmed_finish<<<dim3(1), dim3(1024), 0, st>>>(G, K, labels, near, size, within, cost, n_swaps, status, w.ctl);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_silhouette(const float* dist, int32_t G, int32_t K, const int32_t* labels, double* a, double* b, double* s,
                                 int32_t* other, int32_t* size, double* cluster_mean, double* mean, int32_t* status, uint64_t* work,
                                 void* stream) {
  if (!dist || !labels || !a || !b || !s || !other || !size || !cluster_mean || !mean || !status || !work || G < 0)
    return AGDIFF_ERR_ARG;
  if (K < 1 || K > AGDIFF_PRUNE_MAX_CONFS) return AGDIFF_ERR_ARG;
  if ((uintptr_t)work & 7) return AGDIFF_ERR_ARG;
  if (G > AGDIFF_PRUNE_MAX_CONFS) return AGDIFF_ERR_LIMIT;
  hipStream_t st = (hipStream_t)stream;
  if (G == 0)                                       // no launch: status = 0 and size = 0, mean and cluster_mean NaN
    return ag_fill_outputs({{status, 0, 4}, {size, 0, (size_t)K * 4}, {mean, 0xff, 8}, {cluster_mean, 0xff, (size_t)K * 8}}, st);
  int32_t* ctl = (int32_t*)work;
  int64_t* T = (int64_t*)(work + KM_CTL_WORDS * 4 / 8);
  k_sil_init<<<dim3(1), dim3(1024), 0, st>>>(G, K, labels, a, b, s, other, size, cluster_mean, mean, status, ctl);
  AG_CHECK_LAUNCH();
  const ag_row_launch rows = ag_row_pass_launch(G, K);
  const auto k_rows = rows.wave_rows ? k_sil_rows<4> : k_sil_rows<1>;
  k_rows<<<rows.grid, dim3(256), rows.lds, st>>>(dist, G, K, labels, size, a, b, s, other, T, ctl);
  AG_CHECK_LAUNCH();
  k_sil_finish<<<dim3(1), dim3(1024), 0, st>>>(G, K, labels, T, size, cluster_mean, mean, status, ctl);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_linkage(const float* dist, int32_t G, int32_t method, int32_t anchor, int32_t* left, int32_t* right,
                              double* height, int32_t* size, int32_t* order, int32_t* status, uint64_t* work, void* stream) {
  if (!dist || !left || !right || !height || !size || !order || !status || !work || G < 0) return AGDIFF_ERR_ARG;
  if (method < AGDIFF_LINKAGE_SINGLE || method > AGDIFF_LINKAGE_AVERAGE) return AGDIFF_ERR_ARG;
  if ((uintptr_t)work & 7) return AGDIFF_ERR_ARG;
  if (G > AGDIFF_PRUNE_MAX_CONFS) return AGDIFF_ERR_LIMIT;
  hipStream_t st = (hipStream_t)stream;
  if (G == 0) return ag_fill_outputs({{status, 0, 4}}, st);      // no launch: status = 0
  const ag_link_work w(work);
  const dim3 rows((unsigned)((G + 3) / 4));
  k_link_head<<<dim3(1), dim3(1024), 0, st>>>(dist, G, anchor, w, left, right, height, size, order, status);
  AG_CHECK_LAUNCH();
  k_link_rows<<<rows, dim3(256), 0, st>>>(dist, G, method, w);
  AG_CHECK_LAUNCH();
  for (int it = 0; it < G - 1; ++it) {              // every launch returns at once past the M - 1 merges there are
    k_link_choose<<<dim3(1), dim3(1024), 0, st>>>(w, G, left, right, height, size);
    AG_CHECK_LAUNCH();
    k_link_update<<<rows, dim3(256), 0, st>>>(w, G, method, it);
    AG_CHECK_LAUNCH();
  }
  k_link_order<<<dim3(1), dim3(1024), 0, st>>>(w, G, order);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_linkage_cut(const float* dist, int32_t G, const int32_t* left, const int32_t* right, const double* height,
                                  const int32_t* order, int32_t count, float stop_height, int32_t* medoids, int32_t* labels,
                                  float* near, int32_t* size, double* within, double* cost, int32_t* n_clusters, int32_t* status,
                                  uint64_t* work, void* stream) {
  if (!dist || !left || !right || !height || !order || !medoids || !labels || !near || !size || !within || !cost || !n_clusters ||
      !status || !work || G < 0)
    return AGDIFF_ERR_ARG;
  const bool unbounded = stop_height > 0.0f && stop_height - stop_height != 0.0f;      // +inf
  if (count < 1 || !(unbounded || (stop_height >= 0.0f && stop_height <= (float)AGDIFF_KMEDOIDS_MAX_DIST))) return AGDIFF_ERR_ARG;
  if ((uintptr_t)work & 7) return AGDIFF_ERR_ARG;
  if (G > AGDIFF_PRUNE_MAX_CONFS) return AGDIFF_ERR_LIMIT;
  hipStream_t st = (hipStream_t)stream;
  if (G == 0) return ag_fill_outputs({{n_clusters, 0, 4}, {status, 0, 4}, {cost, 0, 8}}, st);      // no launch
  // Q(T) * 2^-28: the product is exact in fp64 and nearbyint rounds it half to even, as the kernels' Q does
  const double bound = unbounded ? (double)stop_height : __builtin_nearbyint((double)stop_height * 268435456.0) * (1.0 / 268435456.0);
  int32_t* ctl = (int32_t*)work;
  uint64_t* keys = work + KM_CTL_WORDS * 4 / 8;
  k_link_cut<<<dim3(1), dim3(1024), 0, st>>>(G, left, right, height, order, count, bound, medoids, labels, near, size, within, cost,
                                             n_clusters, status, ctl);
  AG_CHECK_LAUNCH();
  k_kmed_costs<<<dim3((unsigned)((G + 3) / 4)), dim3(256), 0, st>>>(dist, G, labels, keys, ctl);
  AG_CHECK_LAUNCH();
  k_link_medoids<<<dim3(1), dim3(1024), 0, st>>>(dist, G, labels, keys, medoids, near, ctl);
  AG_CHECK_LAUNCH();
  k_kmed_finish<<<dim3(1), dim3(1024), 0, st>>>(G, G, labels, near, size, within, cost, n_clusters, status, ctl);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_align_conformers(const float* pos, const int32_t* atom_idx, const float* target, int32_t G, int32_t n, int32_t m,
                                       float* out, float* rmsd, void* stream) {
  if (!pos || !atom_idx || !target || !out || G < 0 || n <= 0 || m <= 0 || m > n) return AGDIFF_ERR_ARG;
  if (G == 0) return AGDIFF_OK;
  k_align_conformers<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, atom_idx, target, n, m, out, rmsd);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_rmsd_matrix_hands(const float* pos_ref, const float* pos_gen, const int32_t* atom_idx, const int32_t* perms,
                                        int32_t R, int32_t G, int32_t n, int32_t m, int32_t P, float* scratch, float* out_proper,
                                        float* out_mirror, void* stream) {
  if (!out_mirror || out_proper == out_mirror) return AGDIFF_ERR_ARG;
  return ag_rmsd_matrix<true>(pos_ref, pos_gen, atom_idx, perms, R, G, n, m, P, scratch, out_proper, out_mirror, stream);
}

extern "C" int agdiff_chiral_verdict(const float* pos, const int32_t* quads, const int8_t* target, int32_t G, int32_t n, int32_t C,
                                     float* vol, int32_t* verdict, void* stream) {
  if (!pos || !verdict || G < 0 || n <= 0 || C < 0 || (C > 0 && (!quads || !target))) return AGDIFF_ERR_ARG;
  if (G == 0) return AGDIFF_OK;
  k_chiral_verdict<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, quads, target, n, C, vol, verdict);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_mirror_conformers(float* pos, const int32_t* flags, int32_t G, int32_t n, void* stream) {
  if (!pos || !flags || G < 0 || n <= 0) return AGDIFF_ERR_ARG;
  if (G == 0) return AGDIFF_OK;
  k_mirror_conformers<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, flags, n);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_flip_double_bonds(float* pos, const int32_t* quads, const int8_t* target, const int32_t* side_ptr,
                                        const int32_t* side_idx, int32_t G, int32_t n, int32_t D, int8_t* state, int32_t* flipped,
                                        void* stream) {
  if (G < 0 || n <= 0 || D < 0) return AGDIFF_ERR_ARG;
  if (G == 0 || D == 0) return AGDIFF_OK;
  if (!pos || !quads || !target || !side_ptr || !state) return AGDIFF_ERR_ARG;
  k_flip_double_bonds<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, quads, target, side_ptr, side_idx, n, D, state, flipped);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_torsion_angles(const float* pos, const int32_t* quads, int32_t G, int32_t n, int32_t Q, float* out, void* stream) {
  if (!pos || !out || G < 0 || n <= 0 || Q < 0 || (Q > 0 && !quads)) return AGDIFF_ERR_ARG;
  if (G == 0 || Q == 0) return AGDIFF_OK;
  k_torsion_angles<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, quads, n, Q, out);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_tfd_matrix(const float* ang_x, const float* ang_y, const int32_t* tmap, const float* w, int32_t R, int32_t G,
                                 int32_t Q, int32_t T, int32_t P, float thresh, float* out, float* out_mirror, uint64_t* bits,
                                 void* stream) {
  if (R < 0 || G < 0 || Q < 0 || T < 0 || T > Q || P < 1 || (Q > 0 && (!ang_x || !ang_y)) || (T > 0 && !tmap)) return AGDIFF_ERR_ARG;
  if ((!out && !out_mirror && !bits) || (out_mirror && out_mirror == out)) return AGDIFF_ERR_ARG;
  if (bits && (!(thresh >= 0.0f) || ((uintptr_t)bits & 7))) return AGDIFF_ERR_ARG;
  if (Q > AGDIFF_TFD_MAX_COLUMNS) return AGDIFF_ERR_LIMIT;
  if (R == 0 || G == 0) return AGDIFF_OK;
  const auto smem_for = [](int q) { return (size_t)2 * 16 * (q | 1) * sizeof(float); };
  static std::atomic<uint64_t> attr_done{0};
  if (smem_for(Q) > 48 * 1024 && !ag_allow_big_lds(attr_done, smem_for(AGDIFF_TFD_MAX_COLUMNS), k_tfd_matrix)) return AGDIFF_ERR_LAUNCH;
  k_tfd_matrix<<<dim3((unsigned)((G + 15) / 16), (unsigned)((R + 15) / 16)), dim3(256), smem_for(Q), (hipStream_t)stream>>>(
      ang_x, ang_y, tmap, w, R, G, Q, T, P, thresh, out, out_mirror, (uint16_t*)bits, ag_bits_pitch(G));
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_ring_coords(const float* pos, const int32_t* ring_ptr, const int32_t* ring_idx, int32_t G, int32_t n, int32_t Rg,
                                  float* tau, float* amp, float* pucker, void* stream) {
  if (!pos || G < 0 || n <= 0 || Rg < 0 || (Rg > 0 && (!ring_ptr || !ring_idx)) || (!tau && !amp && !pucker)) return AGDIFF_ERR_ARG;
  if (G == 0 || Rg == 0) return AGDIFF_OK;
  // the ring sizes, read back in pieces of a fixed host buffer (consecutive pieces share one word): the kernel's passes rely on them
  int32_t host[1024];
  for (int32_t r0 = 0; r0 < Rg; r0 += 1023) {
    const int32_t words = (Rg - r0 < 1023 ? Rg - r0 : 1023) + 1;
    if (hipMemcpyAsync(host, ring_ptr + r0, (size_t)words * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
      (void)hipGetLastError();
      return AGDIFF_ERR_LAUNCH;
    }
    if (r0 == 0 && host[0] != 0) return AGDIFF_ERR_ARG;
    for (int32_t k = 0; k + 1 < words; ++k) {
      const int64_t size = (int64_t)host[k + 1] - host[k];
      if (size < 4 || size > AGDIFF_RING_MAX_ATOMS) return AGDIFF_ERR_LIMIT;
    }
  }
  k_ring_coords<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, ring_ptr, ring_idx, n, Rg, tau, amp, pucker);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_tfd_matrix_terms(const float* ang_x, const float* ang_y, const int32_t* tmap, const float* w, const float* scale,
                                       const int32_t* even, int32_t R, int32_t G, int32_t Q, int32_t T, int32_t P, float thresh,
                                       float* out, float* out_mirror, uint64_t* bits, void* stream) {
  if (R < 0 || G < 0 || Q < 0 || T < 0 || T > Q || P < 1 || (Q > 0 && (!ang_x || !ang_y)) || (T > 0 && (!tmap || !scale || !even)))
    return AGDIFF_ERR_ARG;
  if ((!out && !out_mirror && !bits) || (out_mirror && out_mirror == out)) return AGDIFF_ERR_ARG;
  if (bits && (!(thresh >= 0.0f) || ((uintptr_t)bits & 7))) return AGDIFF_ERR_ARG;
  if (Q > AGDIFF_TFD_MAX_COLUMNS) return AGDIFF_ERR_LIMIT;
  if (R == 0 || G == 0) return AGDIFF_OK;
  const auto smem_for = [](int q, int t) { return (size_t)t * 2 * sizeof(double) + (size_t)2 * 16 * (q | 1) * sizeof(float); };
  static std::atomic<uint64_t> attr_done{0};
  if (smem_for(Q, T) > 48 * 1024 &&
      !ag_allow_big_lds(attr_done, smem_for(AGDIFF_TFD_MAX_COLUMNS, AGDIFF_TFD_MAX_COLUMNS), k_tfd_matrix_terms))
    return AGDIFF_ERR_LAUNCH;
  k_tfd_matrix_terms<<<dim3((unsigned)((G + 15) / 16), (unsigned)((R + 15) / 16)), dim3(256), smem_for(Q, T), (hipStream_t)stream>>>(
      ang_x, ang_y, tmap, w, scale, even, R, G, Q, T, P, thresh, out, out_mirror, (uint16_t*)bits, ag_bits_pitch(G));
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_pair_bounds(const float* pos, const int32_t* pairs, const float* lo, const float* hi, int32_t G, int32_t n, int32_t K,
                                  float* dist, float* worst, int32_t* worst_pair, int32_t* n_bad, void* stream) {
  if (!pos || !worst || !worst_pair || !n_bad || G < 0 || n <= 0 || K < 0 || (K > 0 && (!pairs || !lo || !hi))) return AGDIFF_ERR_ARG;
  if (G == 0) return AGDIFF_OK;
  k_pair_bounds<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, pairs, lo, hi, n, K, dist, worst, worst_pair, n_bad);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_planar_groups(const float* pos, const int32_t* grp_ptr, const int32_t* grp_idx, int32_t G, int32_t n, int32_t P,
                                    float thresh, float* dev, float* worst, int32_t* worst_group, int32_t* n_bent, void* stream) {
  if (!pos || !worst || !worst_group || !n_bent || G < 0 || n <= 0 || P < 0 || (P > 0 && (!grp_ptr || !grp_idx))) return AGDIFF_ERR_ARG;
  if (!(thresh >= 0.0f && thresh <= 3.40282347e38f)) return AGDIFF_ERR_ARG;
  if (G == 0) return AGDIFF_OK;
  k_planar_groups<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, grp_ptr, grp_idx, n, P, thresh, dev, worst, worst_group,
                                                                           n_bent);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_clash_scan(const float* pos, const float* radius, const int32_t* ex_ptr, const int32_t* ex_idx, int32_t G, int32_t n,
                                 float thresh, int32_t* scratch, float* min_ratio, int32_t* min_pair, int32_t* n_clash, void* stream) {
  if (!pos || !radius || !ex_ptr || !scratch || !min_ratio || !min_pair || !n_clash || G < 0 || n <= 0) return AGDIFF_ERR_ARG;
  if (!(thresh >= 0.0f && thresh <= 3.40282347e38f)) return AGDIFF_ERR_ARG;
  if (n > AGDIFF_MAX_ATOMS_LARGE) return AGDIFF_ERR_LIMIT;
  if (G == 0) return AGDIFF_OK;
  hipStream_t st = (hipStream_t)stream;
  const int S = (n + AGDIFF_CLASH_SLICE - 1) / AGDIFF_CLASH_SLICE;
  for (int g0 = 0; g0 < G; g0 += 65535) {           // (a grid's y extent ends at 65535)
    const int gc = G - g0 < 65535 ? G - g0 : 65535;
    k_clash_scan<<<dim3((unsigned)S, (unsigned)gc), dim3(AGDIFF_CLASH_SLICE), 0, st>>>(pos + (size_t)g0 * n * 3, radius, ex_ptr, ex_idx, n,
                                                                                    thresh, scratch + (size_t)g0 * S * 4);
    AG_CHECK_LAUNCH();
  }
  k_clash_finish<<<dim3((unsigned)G), dim3(64), 0, st>>>(scratch, S, min_ratio, min_pair, n_clash);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

// the argument checks and the launch of both repairs; groups == nullptr or P = 0: k_relax_bounds
static int ag_relax_launch(const float* pos, const int32_t* bd_ptr, const int32_t* bd_idx, const float* bd_lo, const float* bd_hi,
                           const float* radius, const int32_t* ex_ptr, const int32_t* ex_idx, int32_t G, int32_t n, int32_t K, float clash,
                           float pad, float omega, int32_t max_iter, const ag_planes_t* groups, float* pos_out, int32_t* status,
                           int32_t* iters, float* resid, float* moved, void* stream) {
  if (!pos || !bd_ptr || !radius || !ex_ptr || !pos_out || !status || !iters || !resid || !moved || pos_out == pos || G < 0 || n <= 0 ||
      K < 0 || (K > 0 && (!bd_idx || !bd_lo || !bd_hi)))
    return AGDIFF_ERR_ARG;
  if (max_iter < 1 || max_iter > AGDIFF_RELAX_MAX_ITERS) return AGDIFF_ERR_ARG;
  if (!(pad > 0.0f && pad <= 3.40282347e38f) || !(omega > 0.0f && omega < 2.0f) || !(clash >= 0.0f && clash <= 3.40282347e38f))
    return AGDIFF_ERR_ARG;
  if (groups) {
    const ag_planes_t& pl = *groups;
    if (pl.P < 0 || (pl.P > 0 && (!pl.grp_ptr || !pl.grp_idx || !pl.mb_ptr || !pl.mb_grp))) return AGDIFF_ERR_ARG;
    if (!(pl.thresh >= 0.0f && pl.thresh <= 3.40282347e38f) || !(pl.flat_to >= 0.0f && pl.flat_to <= 3.40282347e38f))
      return AGDIFF_ERR_ARG;
    if ((double)pl.flat_to + (double)pad > (double)pl.thresh) return AGDIFF_ERR_ARG;
  }
  if (n > AGDIFF_RELAX_MAX_ATOMS || (groups && groups->P > AGDIFF_FLATTEN_MAX_GROUPS)) return AGDIFF_ERR_LIMIT;
  if (G == 0) return AGDIFF_OK;
  int L = 1;                                        // lanes per atom: the largest power of two <= 64 with n L <= 256
  while (L < 64 && 2 * L * n <= AG_RELAX_THREADS) L <<= 1;
  const dim3 grid((unsigned)G), block(AG_RELAX_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (groups && groups->P > 0) {
    if (n <= 128)
      k_relax_planar<128><<<grid, block, 0, st>>>(pos, bd_ptr, bd_idx, bd_lo, bd_hi, radius, ex_ptr, ex_idx, n, L, clash, pad, omega,
                                                  max_iter, *groups, pos_out, status, iters, resid, moved);
    else
      k_relax_planar<AGDIFF_RELAX_MAX_ATOMS><<<grid, block, 0, st>>>(pos, bd_ptr, bd_idx, bd_lo, bd_hi, radius, ex_ptr, ex_idx, n, L, clash,
                                                                     pad, omega, max_iter, *groups, pos_out, status, iters, resid, moved);
  } else if (n <= 128) {
    k_relax_bounds<128><<<grid, block, 0, st>>>(pos, bd_ptr, bd_idx, bd_lo, bd_hi, radius, ex_ptr, ex_idx, n, L, clash, pad, omega, max_iter,
                                                pos_out, status, iters, resid, moved);
  } else {
    k_relax_bounds<AGDIFF_RELAX_MAX_ATOMS><<<grid, block, 0, st>>>(pos, bd_ptr, bd_idx, bd_lo, bd_hi, radius, ex_ptr, ex_idx, n, L, clash,
                                                                   pad, omega, max_iter, pos_out, status, iters, resid, moved);
  }
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_relax_bounds(const float* pos, const int32_t* bd_ptr, const int32_t* bd_idx, const float* bd_lo, const float* bd_hi,
                                   const float* radius, const int32_t* ex_ptr, const int32_t* ex_idx, int32_t G, int32_t n, int32_t K,
                                   float clash, float pad, float omega, int32_t max_iter, float* pos_out, int32_t* status, int32_t* iters,
                                   float* resid, float* moved, void* stream) {
  return ag_relax_launch(pos, bd_ptr, bd_idx, bd_lo, bd_hi, radius, ex_ptr, ex_idx, G, n, K, clash, pad, omega, max_iter, nullptr, pos_out,
                         status, iters, resid, moved, stream);
}

extern "C" int agdiff_relax_planar(const float* pos, const int32_t* bd_ptr, const int32_t* bd_idx, const float* bd_lo, const float* bd_hi,
                                   const float* radius, const int32_t* ex_ptr, const int32_t* ex_idx, const int32_t* grp_ptr,
                                   const int32_t* grp_idx, const int32_t* mb_ptr, const int32_t* mb_grp, int32_t G, int32_t n, int32_t K,
                                   int32_t P, float clash, float pad, float omega, int32_t max_iter, float thresh, float flat_to,
                                   float* pos_out, int32_t* status, int32_t* iters, float* resid, float* moved, void* stream) {
  const ag_planes_t groups = {grp_ptr, grp_idx, mb_ptr, mb_grp, P, thresh, flat_to};
  return ag_relax_launch(pos, bd_ptr, bd_idx, bd_lo, bd_hi, radius, ex_ptr, ex_idx, G, n, K, clash, pad, omega, max_iter, &groups, pos_out,
                         status, iters, resid, moved, stream);
}

extern "C" int agdiff_traj_rmsd(const float* frames, int64_t frame_stride, const float* target, const uint8_t* select,
                                const int32_t* graph_ptr, int32_t S, int32_t G, int32_t N, float* out, float* out_mirror, void* stream) {
  if (!frames || !target || !select || !graph_ptr || !out || out_mirror == out || S < 0 || G < 0 || N <= 0 || frame_stride < (int64_t)3 * N)
    return AGDIFF_ERR_ARG;
  if (S == 0 || G == 0) return AGDIFF_OK;
  hipStream_t st = (hipStream_t)stream;
  for (int s0 = 0; s0 < S; s0 += 65535) {           // (a grid's y extent ends at 65535)
    const int sc = S - s0 < 65535 ? S - s0 : 65535;
    const float* f = frames + (size_t)s0 * frame_stride;
    float* o = out + (size_t)s0 * G;
    if (out_mirror)
      k_traj_rmsd<true><<<dim3((unsigned)G, (unsigned)sc), dim3(64), 0, st>>>(f, frame_stride, target, select, graph_ptr, G, N, o,
                                                                             out_mirror + (size_t)s0 * G);
    else
      k_traj_rmsd<false><<<dim3((unsigned)G, (unsigned)sc), dim3(64), 0, st>>>(f, frame_stride, target, select, graph_ptr, G, N, o, nullptr);
    AG_CHECK_LAUNCH();
  }
  return AGDIFF_OK;
}

extern "C" int agdiff_hold_core(float* pos, const float* core_pos, const uint8_t* select, const int32_t* graph_ptr, const int32_t* skip,
                                int32_t G, int32_t N, float weight, float* copy_out, float* dev, void* stream) {
  if (!pos || !core_pos || !select || !graph_ptr || G < 0 || N <= 0 || !(weight > 0.0f && weight <= 1.0f)) return AGDIFF_ERR_ARG;
  if (copy_out == pos || core_pos == pos || (copy_out && copy_out == core_pos)) return AGDIFF_ERR_ARG;
  if (G == 0) return AGDIFF_OK;
  k_hold_core<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, core_pos, select, graph_ptr, skip, N, weight, copy_out, dev);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_restrain_pairs(float* pos, const int32_t* graph_ptr, const int32_t* rs_ptr, const int32_t* rs_idx, const float* rs_lo,
                                     const float* rs_hi, const uint8_t* fixed, const int32_t* skip, int32_t G, int32_t N, int32_t R2,
                                     int32_t max_restrained, float weight, int32_t sweeps, float* copy_out, float* viol, void* stream) {
  if (!pos || !graph_ptr || !rs_ptr || G < 0 || N <= 0 || R2 < 0 || max_restrained < 0 || !(weight > 0.0f && weight <= 1.0f) ||
      sweeps < 0 || sweeps > 16)
    return AGDIFF_ERR_ARG;
  if (R2 > 0 && (!rs_idx || !rs_lo || !rs_hi)) return AGDIFF_ERR_ARG;
  if (copy_out == pos) return AGDIFF_ERR_ARG;
  if (max_restrained > AGDIFF_RESTRAIN_MAX_ATOMS) return AGDIFF_ERR_LIMIT;
  if (G == 0) return AGDIFF_OK;
  k_restrain_pairs<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, graph_ptr, rs_ptr, rs_idx, rs_lo, rs_hi, fixed, skip, N, R2,
                                                                           weight, sweeps, copy_out, viol);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_restrain_torsions(float* pos, const int32_t* graph_ptr, const int32_t* tr_ptr, const int32_t* quads, const float* centre,
                                        const float* half, const int32_t* side_row, const int32_t* side_ptr, const int32_t* side_idx,
                                        const int32_t* skip, int32_t G, int32_t N, int32_t T, int32_t S, float weight, int32_t turn,
                                        float* copy_out, float* angle, float* viol, void* stream) {
  if (!pos || !graph_ptr || !tr_ptr || !viol || G < 0 || N <= 0 || T < 0 || S < 0 || !(weight > 0.0f && weight <= 1.0f))
    return AGDIFF_ERR_ARG;
  if (T > 0 && (!quads || !centre || !half || !side_row)) return AGDIFF_ERR_ARG;
  if (S > 0 && !side_ptr) return AGDIFF_ERR_ARG;
  if (copy_out == pos) return AGDIFF_ERR_ARG;
  if (G == 0) return AGDIFF_OK;
  k_restrain_torsions<<<dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream>>>(pos, graph_ptr, tr_ptr, quads, centre, half, side_row, side_ptr,
                                                                              side_idx, skip, N, T, S, weight, turn, copy_out, angle, viol);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

// the checks the two MMD calls share; M = R + G <= 2^31 - 2 either way
static int ag_mmd_check(const float* tab_x, const float* tab_y, int32_t R, int32_t G, int32_t K, const void* scratch, const float* mmd2,
                        const float* bandwidth) {
  if (!tab_x || !tab_y || !scratch || !mmd2 || !bandwidth || R < 1 || G < 1 || K < 1 || ((uintptr_t)scratch & 7)) return AGDIFF_ERR_ARG;
  if ((int64_t)R + (int64_t)G > 0x7ffffffell) return AGDIFF_ERR_LIMIT;
  return AGDIFF_OK;
}

extern "C" int agdiff_mmd_all(const float* tab_x, const float* tab_y, int32_t R, int32_t G, int32_t K, void* scratch, float* mmd2,
                              float* bandwidth, void* stream) {
  const int rc = ag_mmd_check(tab_x, tab_y, R, G, K, scratch, mmd2, bandwidth);
  if (rc != AGDIFF_OK) return rc;
  const int64_t T = ((int64_t)R + G + 15) / 16;
  const int64_t tiles = T * (T + 1) / 2;
  if (tiles >= (1ll << 24)) return AGDIFF_ERR_LIMIT;      // (256 threads per tile: the grid stays below 2^32 threads)
  hipStream_t st = (hipStream_t)stream;
  double* scatter = (double*)scratch;               // [K]
  double* bw = scatter + K;                         // [1]
  double* partial = bw + 1;                         // [tiles][3]
  k_mmd_stats<<<dim3((unsigned)(((int64_t)K + 15) / 16)), dim3(256), 0, st>>>(tab_x, tab_y, R, G, K, nullptr, scatter, nullptr, nullptr);
  AG_CHECK_LAUNCH();
  k_mmd_bandwidth<<<dim3(1), dim3(64), 0, st>>>(scatter, K, R + G, bw, bandwidth);
  AG_CHECK_LAUNCH();
  k_mmd_all<<<dim3((unsigned)tiles), dim3(256), 0, st>>>(tab_x, tab_y, R, G, K, (int)T, bw, partial);
  AG_CHECK_LAUNCH();
  k_mmd_all_finish<<<dim3(1), dim3(64), 0, st>>>(partial, (long long)tiles, bw, R, G, mmd2);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}

extern "C" int agdiff_mmd_single(const float* tab_x, const float* tab_y, int32_t R, int32_t G, int32_t K, void* scratch, float* mmd2,
                                 float* bandwidth, void* stream) {
  const int rc = ag_mmd_check(tab_x, tab_y, R, G, K, scratch, mmd2, bandwidth);
  if (rc != AGDIFF_OK) return rc;
  if ((int64_t)R + G > AGDIFF_MMD_MAX_CONFS) return AGDIFF_ERR_LIMIT;
  hipStream_t st = (hipStream_t)stream;
  const int M = R + G;
  double* scatter = (double*)scratch;               // [K]
  double* bw = scatter + K;                         // [K]
  float* zt = (float*)(bw + K);                     // [K][M]
  k_mmd_stats<<<dim3((unsigned)(((int64_t)K + 15) / 16)), dim3(256), 0, st>>>(tab_x, tab_y, R, G, K, zt, scatter, bw, bandwidth);
  AG_CHECK_LAUNCH();
  k_mmd_single<<<dim3((unsigned)K), dim3(AG_MMD_SINGLE_THREADS), (size_t)M * sizeof(float), st>>>(zt, bw, R, G, mmd2);
  AG_CHECK_LAUNCH();
  return AGDIFF_OK;
}
