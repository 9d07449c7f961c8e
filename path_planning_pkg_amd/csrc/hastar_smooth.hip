// hastar_smooth.hip — the clearance field and the batched path smoother.
//
// No reference counterpart: the reference returns the search's arcs as they are.  Both
// products are restated op by op in tests/smoother_ref.py, so every operation below is one
// float32 (or integer) operation in a fixed order; the build's -ffp-contract=off keeps it so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hastar.h"
#include "hastar_device.h"
#include "hastar_smooth.h"

namespace hastar {

// ------------------------------------------------------------------ clearance field ----
// Pass A, along j (the contiguous axis): one workgroup per map row.  The row's occupancy
// flags sit in LDS; every thread owns a run of ceil(N / 256) cells, the runs' last / first
// occupied cells are combined by a 256-entry scan, and each thread then walks its run forward
// (nearest occupied cell at or before j) and backward (at or after j).  Writes |j - j'|, or
// EDT_ROW_NONE for a row with no occupied cell.
__global__ __launch_bounds__(SMOOTH_THREADS) void k_edt_rows(const EdtMap* __restrict__ maps, int N) {
  extern __shared__ int edt_row[];
  __shared__ int c_last[SMOOTH_THREADS], c_first[SMOOTH_THREADS];
  const int t = (int)threadIdx.x, i = (int)blockIdx.x;
  const EdtMap M = maps[blockIdx.y];
  const GAS float* occ = gp(M.occ) + (size_t)i * N;
  for (int j = t; j < N; j += SMOOTH_THREADS) edt_row[j] = occ[j] >= M.thr ? 1 : 0;
  __syncthreads();
  const int C = (N + SMOOTH_THREADS - 1) / SMOOTH_THREADS;
  const int j0 = t * C, j1 = j0 + C < N ? j0 + C : N;
  int last = -1, first = EDT_ROW_NONE;
  for (int j = j0; j < j1; ++j)
    if (edt_row[j]) {
      last = j;
      if (first == EDT_ROW_NONE) first = j;
    }
  c_last[t] = last;
  c_first[t] = first;
  __syncthreads();
  // inclusive prefix maximum of c_last, inclusive suffix minimum of c_first
  for (int o = 1; o < SMOOTH_THREADS; o <<= 1) {
    int a = c_last[t], b = c_first[t];
    if (t >= o && c_last[t - o] > a) a = c_last[t - o];
    if (t + o < SMOOTH_THREADS && c_first[t + o] < b) b = c_first[t + o];
    __syncthreads();
    c_last[t] = a;
    c_first[t] = b;
    __syncthreads();
  }
  int run = t > 0 ? c_last[t - 1] : -1;
  for (int j = j0; j < j1; ++j) {
    if (edt_row[j]) run = j;
    edt_row[j] = run >= 0 ? j - run : EDT_ROW_NONE;  // 0 exactly on the occupied cells
  }
  int nxt = t + 1 < SMOOTH_THREADS ? c_first[t + 1] : EDT_ROW_NONE;
  for (int j = j1 - 1; j >= j0; --j) {
    int v = edt_row[j];
    if (v == 0) nxt = j;
    else if (nxt != EDT_ROW_NONE && nxt - j < v) v = nxt - j;
    edt_row[j] = v;
  }
  __syncthreads();
  GAS int* dst = gp(M.dst) + (size_t)i * N;
  for (int j = t; j < N; j += SMOOTH_THREADS) dst[j] = edt_row[j];
}

// Pass B, along i: one thread per map column (adjacent threads read adjacent j), the lower
// envelope of the parabolas (x - u)^2 + g(u)^2 over the rows u whose pass-A value g(u) is
// finite (Meijster et al. 2000, with the integer separator).  The stack of envelope pieces
// {row s, first row t it covers, g(s)^2} lives in pooled scratch, level-major so that threads
// at the same level touch adjacent words.  Pass-A values are read, then overwritten, by the
// column's own thread.  The outer loops run N times; the pops add up to at most N.
__global__ __launch_bounds__(SMOOTH_THREADS) void k_edt_cols(const EdtMap* __restrict__ maps, int N,
                                                             int* __restrict__ stacks) {
  const int j = (int)(blockIdx.x * SMOOTH_THREADS + threadIdx.x);
  if (j >= N) return;
  const EdtMap M = maps[blockIdx.y];
  GAS int* d = gp(M.dst);
  const size_t NN = (size_t)N * N;
  GAS int* S = gp(stacks) + (size_t)blockIdx.y * 3 * NN;
  GAS int* T = S + NN;
  GAS int* F = T + NN;
  int q = -1, sq = 0, tq = 0;  // the top of the stack, kept in registers
  long long fq = 0;
  for (int u = 0; u < N; ++u) {
    const int g = d[(size_t)u * N + j];
    if (g == EDT_ROW_NONE) continue;
    const long long fu = (long long)g * g;
    while (q >= 0) {
      const long long a = (long long)(tq - sq) * (tq - sq) + fq;
      const long long b = (long long)(tq - u) * (tq - u) + fu;
      if (a <= b) break;
      --q;
      if (q >= 0) {
        const size_t k = (size_t)q * N + j;
        sq = S[k];
        tq = T[k];
        fq = F[k];
      }
    }
    if (q < 0) {
      q = 0;
      sq = u;
      tq = 0;
      fq = fu;
    } else {
      // first row where parabola u is strictly below parabola sq: 1 + floor(num / den)
      const long long num = (long long)u * u - (long long)sq * sq + fu - fq, den = 2ll * (u - sq);
      long long sep = num / den;
      if (num % den != 0 && num < 0) --sep;
      if (sep + 1 >= N) continue;
      ++q;
      sq = u;
      tq = (int)(sep + 1);
      fq = fu;
    }
    const size_t k = (size_t)q * N + j;
    S[k] = sq;
    T[k] = tq;
    F[k] = (int)fq;
  }
  if (q < 0) {  // no occupied cell in this column's map at all
    for (int u = 0; u < N; ++u) d[(size_t)u * N + j] = HASTAR_CLEAR_NONE;
    return;
  }
  for (int u = N - 1; u >= 0; --u) {
    d[(size_t)u * N + j] = (int)((long long)(u - sq) * (u - sq) + fq);
    if (u == tq && q > 0) {
      --q;
      const size_t k = (size_t)q * N + j;
      sq = S[k];
      tq = T[k];
      fq = F[k];
    }
  }
}

hipError_t launch_edt(const EdtMap* d_maps, int nmaps, int N, int* d_stacks, hipStream_t st) {
  if (nmaps <= 0) return hipSuccess;
  const size_t lds = (size_t)N * sizeof(int);
  // the dynamic-LDS opt-in, once per device (callers hold the device context's lock)
  static bool attr[64] = {};
  int dev = 0;
  hipError_t a = hipGetDevice(&dev);
  if (a != hipSuccess) return a;
  if (!attr[dev & 63]) {
    a = hipFuncSetAttribute(reinterpret_cast<const void*>(k_edt_rows), hipFuncAttributeMaxDynamicSharedMemorySize,
                            EDT_MAX_N * (int)sizeof(int));
    if (a != hipSuccess) return a;
    attr[dev & 63] = true;
  }
  hipLaunchKernelGGL(k_edt_rows, dim3(N, nmaps), dim3(SMOOTH_THREADS), lds, st, d_maps, N);
  a = hipGetLastError();
  if (a != hipSuccess) return a;
  hipLaunchKernelGGL(k_edt_cols, dim3((N + SMOOTH_THREADS - 1) / SMOOTH_THREADS, nmaps), dim3(SMOOTH_THREADS), 0, st,
                     d_maps, N, d_stacks);
  return hipGetLastError();
}

// ------------------------------------------------------------------------- smoother ----
__device__ __forceinline__ float block_max(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// clearance of one cell in metres; a map without obstacles counts as d_max away
__device__ __forceinline__ float clear_cell(const GAS int* d2, int N, int i, int j, float res, float d_max) {
  const int v = d2[(size_t)i * N + j];
  return v == HASTAR_CLEAR_NONE ? d_max : res * sqrtf((float)v);
}
// a cell coordinate (already floored, as float) clamped into [0, N - 1]; NaN goes to 0
__device__ __forceinline__ int clamp_cell(float f, int N) {
  if (!(f >= 0.0f)) return 0;
  if (f > (float)(N - 1)) return N - 1;
  return (int)f;
}
// Menger curvature of three points: 2 |ab x bc| / (|ab| |bc| |ac|); 0 for coincident points
__device__ __forceinline__ float menger(float ax, float ay, float bx, float by, float cx, float cy) {
  const float abx = bx - ax, aby = by - ay, bcx = cx - bx, bcy = cy - by, acx = cx - ax, acy = cy - ay;
  const float cr = fabsf(abx * bcy - aby * bcx);
  const float l1 = sqrtf(abx * abx + aby * aby), l2 = sqrtf(bcx * bcx + bcy * bcy), l3 = sqrtf(acx * acx + acy * acy);
  const float den = (l1 * l2) * l3;
  return den > 0.0f ? (cr + cr) / den : 0.0f;
}

// One workgroup per path.  Dynamic LDS: two {x[n], y[n]} buffers (16 B per point).
__global__ __launch_bounds__(SMOOTH_THREADS) void k_smooth(
    const SmoothMap* __restrict__ maps, const int* __restrict__ map_of, const long long* __restrict__ off, int p0,
    const float* __restrict__ xyh, const float* __restrict__ curv, const signed char* __restrict__ dir,
    float* __restrict__ xyh_out, float* __restrict__ curv_out, float* __restrict__ g0, float* __restrict__ blend,
    int* __restrict__ status, SmoothParams sp) {
  extern __shared__ float sm_dyn[];
  __shared__ unsigned char fixedm[HASTAR_SMOOTH_MAX_POINTS];
  __shared__ float red[4];
  const int p = p0 + (int)blockIdx.x, t = (int)threadIdx.x;
  const long long base = off[p];
  const long long n_ll = off[p + 1] - base;
  const GAS float* in = gp(xyh) + 3 * base;
  const GAS float* cin = gp(curv) + base;
  GAS float* out = gp(xyh_out) + 3 * base;
  GAS float* cout = gp(curv_out) + base;
  if (n_ll < 5 || n_ll > HASTAR_SMOOTH_MAX_POINTS) {  // copied through
    for (long long i = t; i < n_ll; i += SMOOTH_THREADS) {
      out[3 * i] = in[3 * i];
      out[3 * i + 1] = in[3 * i + 1];
      out[3 * i + 2] = in[3 * i + 2];
      cout[i] = cin[i];
    }
    if (t == 0) {
      blend[p] = 0.0f;
      status[p] = n_ll > HASTAR_SMOOTH_MAX_POINTS ? HASTAR_ENOSPC : 0;
    }
    return;
  }
  const int n = (int)n_ll;
  const SmoothMap M = maps[map_of[p]];
  const GAS signed char* dr = dir ? gp(dir) + base : nullptr;
  GAS float* x0 = gp(g0) + 2 * base;
  const GAS int* d2 = gp(M.d2);
  const GAS float* occ = gp(M.occ);
  const int N = M.N;
  const float res = M.res;
  float* cx = sm_dyn;
  float* cy = sm_dyn + n;
  float* nx = sm_dyn + 2 * n;
  float* ny = sm_dyn + 3 * n;

  // ---- load: world -> grid frame (the inverse of the search's rotate-back), fixed points
  for (int i = t; i < n; i += SMOOTH_THREADS) {
    const float dx = in[3 * i] - M.world_goal_x, dy = in[3 * i + 1] - M.world_goal_y;
    const float gx = (dx * M.rot_c - dy * M.rot_s) + M.goal_x;
    const float gy = (dx * M.rot_s + dy * M.rot_c) + M.goal_y;
    cx[i] = nx[i] = gx;
    cy[i] = ny[i] = gy;
    x0[2 * i] = gx;
    x0[2 * i + 1] = gy;
    fixedm[i] = (i < 2 || i >= n - 2) ? 1 : 0;
  }
  __syncthreads();
  if (dr) {
    for (int i = t; i < n - 1; i += SMOOTH_THREADS)
      if (dr[i] != dr[i + 1]) {  // a cusp: i and its neighbours stay
        if (i > 0) fixedm[i - 1] = 1;
        fixedm[i] = 1;
        fixedm[i + 1] = 1;
      }
    __syncthreads();
  }
  // ---- the input's largest gap and largest curvature over the points that may move
  float gap_in = 0.0f, kap_in = 0.0f;
  for (int i = t; i < n; i += SMOOTH_THREADS) {
    if (i + 1 < n) {
      const float ex = cx[i + 1] - cx[i], ey = cy[i + 1] - cy[i];
      gap_in = fmaxf(gap_in, sqrtf(ex * ex + ey * ey));
    }
    if (!fixedm[i]) kap_in = fmaxf(kap_in, menger(cx[i - 1], cy[i - 1], cx[i], cy[i], cx[i + 1], cy[i + 1]));
  }
  gap_in = block_max(gap_in, red);
  kap_in = block_max(kap_in, red);
  const float gap_lim = 1.25f * gap_in;
  const float kap_lim = fmaxf(M.kappa_max, kap_in);

  // ---- Jacobi gradient descent: read (cx, cy), write (nx, ny), barrier, swap
  for (int it = 0; it < sp.iterations; ++it) {
    for (int i = t; i < n; i += SMOOTH_THREADS) {
      if (fixedm[i]) continue;  // both buffers hold the input there
      const float x = cx[i], y = cy[i];
      // smoothness: D(k) = x[k-1] - 2 x[k] + x[k+1]; d/dx[i] of sum |D|^2 = 2 (D(i-1) - 2 D(i) + D(i+1))
      const float dmx = (cx[i - 2] + x) - (cx[i - 1] + cx[i - 1]);
      const float d0x = (cx[i - 1] + cx[i + 1]) - (x + x);
      const float dpx = (x + cx[i + 2]) - (cx[i + 1] + cx[i + 1]);
      const float dmy = (cy[i - 2] + y) - (cy[i - 1] + cy[i - 1]);
      const float d0y = (cy[i - 1] + cy[i + 1]) - (y + y);
      const float dpy = (y + cy[i + 2]) - (cy[i + 1] + cy[i + 1]);
      const float gsx = sp.ws2 * ((dmx + dpx) - (d0x + d0x));
      const float gsy = sp.ws2 * ((dmy + dpy) - (d0y + d0y));
      // fidelity
      const float gfx = sp.wf2 * (x - x0[2 * i]);
      const float gfy = sp.wf2 * (y - x0[2 * i + 1]);
      // obstacle: the bilinear patch of the clearance between cell centres (cell i at i * res)
      const float u = x / res, v = y / res;
      const float fi = floorf(u), fj = floorf(v);
      const float fu = u - fi, fv = v - fj;
      const int i0 = clamp_cell(fi, N), i1 = clamp_cell(fi + 1.0f, N);
      const int j0 = clamp_cell(fj, N), j1 = clamp_cell(fj + 1.0f, N);
      const float c00 = clear_cell(d2, N, i0, j0, res, sp.d_max), c01 = clear_cell(d2, N, i0, j1, res, sp.d_max);
      const float c10 = clear_cell(d2, N, i1, j0, res, sp.d_max), c11 = clear_cell(d2, N, i1, j1, res, sp.d_max);
      const float a0 = c00 + fv * (c01 - c00), a1 = c10 + fv * (c11 - c10);
      const float b0 = c00 + fu * (c10 - c00), b1 = c01 + fu * (c11 - c01);
      const float c = a0 + fu * (a1 - a0);
      const float m = c < sp.d_max ? sp.wo2 * (sp.d_max - c) : 0.0f;
      const float gox = m * ((a1 - a0) / res), goy = m * ((b1 - b0) / res);
      nx[i] = x - sp.alpha * ((gsx + gfx) - gox);
      ny[i] = y - sp.alpha * ((gsy + gfy) - goy);
    }
    __syncthreads();
    float* sx = cx;
    cx = nx;
    nx = sx;
    float* sy = cy;
    cy = ny;
    ny = sy;
  }

  // ---- accept by blending: the first lambda whose path the map and the vehicle accept
  float lam = 1.0f, accepted = 0.0f;
  for (int k = 0; k < 4; ++k, lam *= 0.5f) {
    for (int i = t; i < n; i += SMOOTH_THREADS) {
      if (fixedm[i]) continue;
      const float ox = x0[2 * i], oy = x0[2 * i + 1];
      nx[i] = ox + lam * (cx[i] - ox);
      ny[i] = oy + lam * (cy[i] - oy);
    }
    __syncthreads();
    float bad = 0.0f, gap = 0.0f, kap = 0.0f;
    const float hi = (float)(N - 1);
    for (int i = t; i < n; i += SMOOTH_THREADS) {
      if (i + 1 < n) {
        const float ex = nx[i + 1] - nx[i], ey = ny[i + 1] - ny[i];
        gap = fmaxf(gap, sqrtf(ex * ex + ey * ey));
      }
      if (fixedm[i]) continue;
      kap = fmaxf(kap, menger(nx[i - 1], ny[i - 1], nx[i], ny[i], nx[i + 1], ny[i + 1]));
      const float u = nx[i] / res, v = ny[i] / res;
      const float fi = floorf(u), fj = floorf(v), ri = roundf(u), rj = roundf(v);
      bool ok = fi >= 0.0f && fi <= hi && fj >= 0.0f && fj <= hi && ri >= 0.0f && ri <= hi && rj >= 0.0f && rj <= hi;
      if (ok)
        ok = !(occ[(size_t)(int)fi * N + (int)fj] >= M.thr) && !(occ[(size_t)(int)ri * N + (int)rj] >= M.thr);
      if (!ok) bad = 1.0f;
    }
    bad = block_max(bad, red);
    gap = block_max(gap, red);
    kap = block_max(kap, red);
    if (bad == 0.0f && gap <= gap_lim && kap <= kap_lim) {
      accepted = lam;
      break;
    }
    __syncthreads();  // the next lambda overwrites (nx, ny)
  }
  if (t == 0) {
    blend[p] = accepted;
    status[p] = 0;
  }
  if (accepted == 0.0f) {  // the input, bit for bit
    for (int i = t; i < n; i += SMOOTH_THREADS) {
      out[3 * i] = in[3 * i];
      out[3 * i + 1] = in[3 * i + 1];
      out[3 * i + 2] = in[3 * i + 2];
      cout[i] = cin[i];
    }
    return;
  }
  // ---- store: grid -> world frame into (cx, cy); fixed points keep their input bits
  __syncthreads();
  for (int i = t; i < n; i += SMOOTH_THREADS) {
    if (fixedm[i]) {
      cx[i] = in[3 * i];
      cy[i] = in[3 * i + 1];
    } else {
      const float ax = nx[i] - M.goal_x, ay = ny[i] - M.goal_y;
      float xr = ax * M.rot_c + ay * M.rot_s;
      float yr = -ax * M.rot_s + ay * M.rot_c;
      xr += M.world_goal_x;
      yr += M.world_goal_y;
      cx[i] = xr;
      cy[i] = yr;
    }
  }
  __syncthreads();
  for (int i = t; i < n; i += SMOOTH_THREADS) {
    out[3 * i] = cx[i];
    out[3 * i + 1] = cy[i];
    if (fixedm[i]) {
      out[3 * i + 2] = in[3 * i + 2];
    } else {
      // the direction of travel: start -> goal is decreasing i
      float h = g_atan2f(cy[i - 1] - cy[i + 1], cx[i - 1] - cx[i + 1]);
      if (dr && dr[i] < 0) h = h > 0.0f ? h - (float)M_PI : h + (float)M_PI;
      out[3 * i + 2] = h;
    }
    const int c = i == 0 ? 1 : (i == n - 1 ? n - 2 : i);  // the end points copy their neighbour
    cout[i] = menger(cx[c - 1], cy[c - 1], cx[c], cy[c], cx[c + 1], cy[c + 1]);
  }
}

hipError_t launch_smooth(const SmoothMap* d_maps, const int* d_map_of, const long long* d_off, int p0, int np,
                         int max_points, const float* xyh, const float* curv, const signed char* dir, float* xyh_out,
                         float* curv_out, float* g0, float* blend, int* status, const SmoothParams& sp,
                         hipStream_t st) {
  if (np <= 0) return hipSuccess;
  static bool attr[64] = {};
  int dev = 0;
  hipError_t a = hipGetDevice(&dev);
  if (a != hipSuccess) return a;
  if (!attr[dev & 63]) {
    a = hipFuncSetAttribute(reinterpret_cast<const void*>(k_smooth), hipFuncAttributeMaxDynamicSharedMemorySize,
                            HASTAR_SMOOTH_MAX_POINTS * 16);
    if (a != hipSuccess) return a;
    attr[dev & 63] = true;
  }
  if (max_points > HASTAR_SMOOTH_MAX_POINTS) max_points = HASTAR_SMOOTH_MAX_POINTS;
  if (max_points < 1) max_points = 1;
  hipLaunchKernelGGL(k_smooth, dim3(np), dim3(SMOOTH_THREADS), (size_t)max_points * 16, st, d_maps, d_map_of, d_off,
                     p0, xyh, curv, dir, xyh_out, curv_out, g0, blend, status, sp);
  return hipGetLastError();
}

}  // namespace hastar
