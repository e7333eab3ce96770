// PowerSGD low-rank compression with error feedback: the kernels of
// bpsr_powersgd.h (the definition is prophet_amd/powersgd.py).
//
//   PROJECT-P      M = g + R over R (one f32 add, pinned); partial M Q tiles
//   REDUCE         the partial tiles of a segment added up in chunk order
//   ORTHOGONALIZE  modified Gram-Schmidt over P's columns, float64 sums
//   PROJECT-Q      partial M^T P tiles over R
//   FINISH         out = P Q^T in the definition's order; R' = M - out (pinned)
//
// Both projections run on v_mfma_f32_16x16x4_f32, whose inputs are exact f32:
// D[16 x 16] += A[16 x 4] B[4 x 16], lane l holding A[l % 16][l / 16],
// B[l / 16][l % 16] and, in four registers v, D[4 (l / 16) + v][l % 16].  The
// rank is padded with zeros to the tile's 16 columns.  The order of a
// projection's additions is the kernels' own: partial tiles per chunk of the
// contraction, then a fixed-order sum — no atomics, so the same bytes in give
// the same bytes out.
//
// PROJECT-P contracts along M's contiguous dimension.  A wave owns 16 rows;
// lane l loads 16 bytes of row l % 16 at column k0 + 4 (l / 16): its four
// values are four A operands, and the MFMA that takes value s pairs it with Q
// row k0 + 4 (l / 16) + s in the same lane — the k index is permuted alike in
// both operands, which a contraction allows.  Four such loads a step cover 64
// columns, 256 contiguous bytes a row.  The workgroup's chunk of Q sits in LDS
// in operand order, 16 floats a column, so a lane's four B values of a load are
// one ds_read_b128 without bank conflicts.
//
// PROJECT-Q contracts over rows, so a 16-byte load along a row holds four
// columns of ONE k: lane l loads row i0 + l / 16, columns c0 + 4 (l % 16) + e,
// and MFMA e accumulates the strided column set {c0 + 4 j + e}.  A wave owns 64
// columns (256 contiguous bytes a row), four accumulators; the B operand, one
// value of P a lane, is shared by the four.
//
// FINISH is element-wise on VALU: the tile's Qn columns ([k][column], b128
// reads) and P rows (one address a wave: a broadcast) sit in LDS.
//
// Partial tiles are guarded in the kernels: a row, a column or a rank index
// past the matrix is not read and enters as +0.0.
#include <algorithm>

#include "bpsr_powersgd.h"

namespace bpsr {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 mfma(float a, float b, f4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Four floats of a row at `at`, columns k .. k + 3 of which those below `end`
// exist: one b128 load where the row is aligned and whole, else element loads.
// NT: a nontemporal load.  Measured per kernel: g and the R
// that PROJECT-Q and FINISH sweep are faster with the hint, the R that PROJECT-P
// reads and writes back in the same step is faster without it.
template <bool NT>
__device__ __forceinline__ f4 load4(const float* at, uint32_t k, uint32_t end, bool vec) {
  f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (vec && k + 4 <= end) {
    const f4* const p = reinterpret_cast<const f4*>(at);
    v = NT ? __builtin_nontemporal_load(p) : *p;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < end) v[e] = NT ? __builtin_nontemporal_load(at + e) : at[e];
  }
  return v;
}

__device__ __forceinline__ void store4(float* at, f4 v, uint32_t k, uint32_t end, bool vec) {
  if (vec && k + 4 <= end) {
    *reinterpret_cast<f4*>(at) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k + e < end) at[e] = v[e];
  }
}

__device__ __forceinline__ bool finite(float x) {
  return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
}

}  // namespace

__global__ __launch_bounds__(kBlock) void psgd_project_p_kernel(PsgdArgs p) {
  // the chunk's Q rows in operand order: [16-column group][lane][s]
  __shared__ __attribute__((aligned(16))) float sq[kPsgdKcMax * 16];
  const PsgdRec rec = p.recs[blockIdx.x];
  const PsgdSeg& S = p.segs[rec.seg];
  const uint32_t n = S.n, m = S.m, r = S.r;
  const bool vec = S.vec != 0;
  const uint32_t k_begin = rec.b * S.kc;
  const uint32_t k_end = k_begin + S.kc < m ? k_begin + S.kc : m;
  const uint32_t steps = (k_end - k_begin + kPsgdKStep - 1) / kPsgdKStep;
  const float* const Q = S.Q;
  // every group a step reads is staged, zeros past the chunk and past the rank
  for (uint32_t it = threadIdx.x; it < steps * 4 * 64; it += kBlock) {
    const uint32_t l = it % 64, k = k_begin + (it / 64) * 16 + 4 * (l / 16), j = l % 16;
    f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (j < r) {
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (k + s < k_end) v[s] = Q[(uint64_t)(k + s) * r + j];
    }
    *reinterpret_cast<f4*>(&sq[it * 4]) = v;
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const uint32_t row0 = rec.a * kPsgdPRows + wave * 16;
  if (row0 >= n) return;
  const uint32_t row = row0 + lane % 16, kg = lane / 16;
  const bool live = row < n;
  const float* const g = S.g + (uint64_t)row * m;
  float* const R = S.R + (uint64_t)row * m;
  f4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = acc0;
  for (uint32_t st = 0; st < steps; ++st) {
    f4 a[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t k = k_begin + st * kPsgdKStep + 16 * t + 4 * kg;
      a[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      if (live && k < k_end)
        a[t] = load4<true>(g + k, k, k_end, vec) + load4<false>(R + k, k, k_end, vec);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const uint32_t k = k_begin + st * kPsgdKStep + 16 * t + 4 * kg;
      if (live && k < k_end) store4(R + k, a[t], k, k_end, vec);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f4 b = *reinterpret_cast<const f4*>(&sq[((st * 4 + t) * 64 + lane) * 4]);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (t & 1)
          acc1 = mfma(a[t][s], b[s], acc1);
        else
          acc0 = mfma(a[t][s], b[s], acc0);
      }
    }
  }
  const f4 acc = acc0 + acc1;
  const uint32_t j = lane % 16;
  float* const part = S.scratch + (uint64_t)rec.b * n * r;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const uint32_t i = row0 + 4 * kg + v;
    if (i < n && j < r) part[(uint64_t)i * r + j] = acc[v];
  }
}

__global__ __launch_bounds__(kBlock) void psgd_project_q_kernel(PsgdArgs p) {
  constexpr int kRows = kPsgdRStep / 4;  // loads in flight a lane
  const PsgdRec rec = p.recs[blockIdx.x];
  const PsgdSeg& S = p.segs[rec.seg];
  const uint32_t n = S.n, m = S.m, r = S.r;
  const bool vec = S.vec != 0;
  const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const uint32_t c0 = rec.a * kPsgdQCols + wave * 64;
  if (c0 >= m) return;
  const uint32_t i_begin = rec.b * S.rc;
  const uint32_t i_end = i_begin + S.rc < n ? i_begin + S.rc : n;
  const uint32_t kg = lane / 16, j = lane % 16, c = c0 + 4 * j;
  const float* const R = S.R;
  const float* const P = S.P;
  f4 acc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t i0 = i_begin; i0 < i_end; i0 += kPsgdRStep) {
    f4 a[kRows];
    float b[kRows];
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      const uint32_t i = i0 + 4 * u + kg;
      a[u] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      b[u] = 0.0f;
      if (i < i_end) {
        if (c < m) a[u] = load4<true>(R + (uint64_t)i * m + c, c, m, vec);
        if (j < r) b[u] = P[(uint64_t)i * r + j];
      }
    }
#pragma unroll
    for (int u = 0; u < kRows; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = mfma(a[u][e], b[u], acc[e]);
  }
  // D_e[jj][j] is column c0 + 4 jj + e, jj = 4 kg + v
  float* const part = S.scratch + (uint64_t)rec.b * m * r;
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const uint32_t col = c0 + 4 * (4 * kg + v) + e;
      if (col < m && j < r) part[(uint64_t)col * r + j] = acc[e][v];
    }
}

// grid (x, segment): dest[i] = part_0[i] + part_1[i] + ..., in that order.
template <bool Q>
__global__ __launch_bounds__(kBlock) void psgd_reduce_kernel(PsgdArgs p) {
  const PsgdSeg& S = p.segs[blockIdx.y];
  const uint64_t count = (uint64_t)(Q ? S.m : S.n) * S.r;
  const uint32_t chunks = Q ? S.qchunks : S.pchunks;
  float* const dst = Q ? S.Qn : S.P;
  const float* const part = S.scratch;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count;
       i += (uint64_t)gridDim.x * kBlock) {
    float s = part[i];
    for (uint32_t ch = 1; ch < chunks; ++ch) s += part[(uint64_t)ch * count + i];
    dst[i] = s;
  }
}

namespace {

// The sum of v over the workgroup, in every thread: a lane's value, the wave's
// xor tree, then the four waves in order — the same order at every call.
__device__ __forceinline__ double block_sum(double v, double* sm) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if (threadIdx.x % 64 == 0) sm[threadIdx.x / 64] = v;
  __syncthreads();
  const double t = ((sm[0] + sm[1]) + sm[2]) + sm[3];
  __syncthreads();
  return t;
}

}  // namespace

// One workgroup a segment.  A thread owns rows tid, tid + 256, ... in every
// column, so a column update needs no barrier of its own: block_sum's are the
// only ones.
__global__ __launch_bounds__(kBlock) void psgd_orthogonalize_kernel(PsgdArgs p) {
  __shared__ double sm[kBlock / 64];
  const PsgdSeg& S = p.segs[blockIdx.x];
  const uint32_t n = S.n, r = S.r;
  float* const P = S.P;
  for (uint32_t k = 0; k < r; ++k) {
    for (uint32_t j = 0; j < k; ++j) {
      double d = 0.0;
      for (uint32_t i = threadIdx.x; i < n; i += kBlock)
        d += (double)P[(uint64_t)i * r + j] * (double)P[(uint64_t)i * r + k];
      d = block_sum(d, sm);
      for (uint32_t i = threadIdx.x; i < n; i += kBlock)
        P[(uint64_t)i * r + k] =
            (float)((double)P[(uint64_t)i * r + k] - d * (double)P[(uint64_t)i * r + j]);
    }
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
      const double x = (double)P[(uint64_t)i * r + k];
      s += x * x;
    }
    s = block_sum(s, sm);
    // 0, inf or NaN: the column is dropped
    const bool ok = s > 0.0 && s < __builtin_huge_val();
    const double nrm = __builtin_sqrt(s);
    for (uint32_t i = threadIdx.x; i < n; i += kBlock)
      P[(uint64_t)i * r + k] = ok ? (float)((double)P[(uint64_t)i * r + k] / nrm) : 0.0f;
  }
}

__global__ __launch_bounds__(kBlock) void psgd_finish_kernel(PsgdArgs p) {
  __shared__ __attribute__((aligned(16))) float sq[kPsgdMaxRank * kPsgdFCols];  // [k][column]
  __shared__ float sp[kPsgdFRows * kPsgdMaxRank];                               // [row][k]
  const PsgdRec rec = p.recs[blockIdx.x];
  const PsgdSeg& S = p.segs[rec.seg];
  const uint32_t n = S.n, m = S.m, r = S.r;
  const bool vec = S.vec != 0;
  const uint32_t i0 = rec.a * kPsgdFRows, c0 = rec.b * kPsgdFCols;
  for (uint32_t it = threadIdx.x; it < kPsgdFCols * r; it += kBlock) {
    const uint32_t cl = it / r, k = it % r;  // Qn's own order: coalesced
    sq[k * kPsgdFCols + cl] = c0 + cl < m ? S.Qn[(uint64_t)(c0 + cl) * r + k] : 0.0f;
  }
  for (uint32_t it = threadIdx.x; it < kPsgdFRows * r; it += kBlock) {
    const uint32_t il = it / r, k = it % r;
    sp[il * kPsgdMaxRank + k] = i0 + il < n ? S.P[(uint64_t)(i0 + il) * r + k] : 0.0f;
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  const uint32_t c = c0 + 4 * lane;
  if (c >= m) return;
  constexpr int kRows = kPsgdFRows / 4;  // a wave's rows: wave, wave + 4, ...
  f4 x[kRows];
#pragma unroll
  for (int u = 0; u < kRows; ++u) {
    const uint32_t i = i0 + wave + 4 * u;
    x[u] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    if (i < n) x[u] = load4<true>(S.R + (uint64_t)i * m + c, c, m, vec);
  }
#pragma unroll
  for (int u = 0; u < kRows; ++u) {
    const uint32_t il = wave + 4 * u, i = i0 + il;
    if (i >= n) break;
    f4 a = {0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t k = 0; k < r; ++k) {
      const float pk = sp[il * kPsgdMaxRank + k];
      const f4 q = *reinterpret_cast<const f4*>(&sq[k * kPsgdFCols + 4 * lane]);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = a[e] + pk * q[e];  // a multiply, then an add
    }
    f4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = finite(a[e]) && finite(x[u][e]) ? x[u][e] - a[e] : 0.0f;
    store4(S.out + (uint64_t)i * m + c, a, c, m, vec);
    store4(S.R + (uint64_t)i * m + c, y, c, m, vec);
  }
}

hipError_t launch_psgd_project_p(const PsgdArgs& a, hipStream_t s) {
  if (a.nrecs == 0) return hipSuccess;
  hipLaunchKernelGGL(psgd_project_p_kernel, dim3(a.nrecs), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_psgd_project_q(const PsgdArgs& a, hipStream_t s) {
  if (a.nrecs == 0) return hipSuccess;
  hipLaunchKernelGGL(psgd_project_q_kernel, dim3(a.nrecs), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_psgd_finish(const PsgdArgs& a, hipStream_t s) {
  if (a.nrecs == 0) return hipSuccess;
  hipLaunchKernelGGL(psgd_finish_kernel, dim3(a.nrecs), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_psgd_reduce(const PsgdArgs& a, bool q, uint64_t most, hipStream_t s) {
  if (a.nsegs == 0) return hipSuccess;
  const uint32_t gx = (uint32_t)std::min<uint64_t>(64, (most + kBlock - 1) / kBlock);
  const dim3 grid(gx ? gx : 1, a.nsegs);
  if (q)
    hipLaunchKernelGGL(psgd_reduce_kernel<true>, grid, dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL(psgd_reduce_kernel<false>, grid, dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_psgd_orthogonalize(const PsgdArgs& a, hipStream_t s) {
  if (a.nsegs == 0) return hipSuccess;
  hipLaunchKernelGGL(psgd_orthogonalize_kernel, dim3(a.nsegs), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace bpsr
