// ssd_agent_tie.hip -- heads shared across agents (include/ssd_hip_tie.h: ssd_tie_agent_grads, ssd_agent_spread; config key share_heads).
//
// Every agent stores its own copy of both heads, [1, n, in, out].  If the n copies of a tensor start equal and receive the same gradient,
// the clip (one global factor), Adam and the Polyak update -- all elementwise -- keep them equal to the bit, so tying the GRADIENTS is the
// whole mechanism: k_tie_agent_grads sums the n gradient slices of every tied tensor in ascending agent order (f32, one rounding per add)
// and writes the sum to all of them, in the flat gradient buffer, in front of the clip.  k_agent_spread measures how far the copies of
// the parameters themselves lie from their mean (logged with the key off too, where it is the interesting number).
//
// Both are bandwidth-trivial (1.3 - 2.5 MB) and sit at the launch floor; they are built for a stated order, not for speed.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ssd_hip_tie.h"
#include "ssd_device.h"

namespace ssd {

constexpr int kTieThreads = 256;
constexpr int kTieMaxBlocksX = 8;       // workgroups along a job's elements (a grid-stride loop takes the rest)

// s = (..((p[0] + p[stride]) + p[2 stride]) ..) over `copies` slices, written back to all of them.  The loads do not depend on each other:
// all are issued before the first add.
template <typename V>
__device__ __forceinline__ V add_in_order(V a, V b);
template <>
__device__ __forceinline__ float add_in_order<float>(float a, float b) { return a + b; }
template <>
__device__ __forceinline__ float4 add_in_order<float4>(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

template <typename V>
__device__ __forceinline__ void tie_copies(V* p, long stride, int copies) {
    V v[SSD_MAX_AGENTS];
#pragma unroll
    for (int i = 0; i < SSD_MAX_AGENTS; ++i)
        if (i < copies) v[i] = p[i * stride];
    V s = v[0];
#pragma unroll
    for (int i = 1; i < SSD_MAX_AGENTS; ++i)
        if (i < copies) s = add_in_order(s, v[i]);
#pragma unroll
    for (int i = 0; i < SSD_MAX_AGENTS; ++i)
        if (i < copies) p[i * stride] = s;
}

// grid (x, job).  A job whose inner is a multiple of 4 has every copy at the same residue of 16 bytes: the elements between the first
// and the last 16-byte boundary of a copy go as float4 (slots 0 .. nvec - 1), the head + tail elements in front of and behind them
// (together 0 or 4) one per thread.  Any other job goes one element per thread, neighbours in neighbouring lanes.
__global__ __launch_bounds__(kTieThreads) void k_tie_agent_grads(float* flat, const int64_t* __restrict__ jobs) {
    const int64_t* j = jobs + 3 * blockIdx.y;
    const long inner = j[2];
    const int copies = (int)j[1];
    float* base = flat + j[0];
    const long first = (long)blockIdx.x * kTieThreads + threadIdx.x, step = (long)gridDim.x * kTieThreads;
    if ((inner & 3) == 0) {
        const long head = (4 - (long)(((uintptr_t)base >> 2) & 3)) & 3;
        const long nvec = (inner - head) >> 2, tail0 = head + 4 * nvec;
        const long slots = nvec + (head ? 4 : 0);
        for (long q = first; q < slots; q += step) {
            if (q < nvec) {
                tie_copies(reinterpret_cast<float4*>(base + head + 4 * q), inner >> 2, copies);
            } else {
                const long k = q - nvec;
                tie_copies(base + (k < head ? k : tail0 + (k - head)), inner, copies);
            }
        }
    } else {
        for (long e = first; e < inner; e += step) tie_copies(base + e, inner, copies);
    }
}

// one workgroup per job; the order of every sum is the header's
__global__ __launch_bounds__(256) void k_agent_spread(const int64_t* __restrict__ jobs, double* __restrict__ out) {
    __shared__ double red[2][256];
    const int64_t* j = jobs + 3 * blockIdx.x;
    const float* base = reinterpret_cast<const float*>((uintptr_t)j[0]);
    const int copies = (int)j[1];
    const long inner = j[2];
    const int t = threadIdx.x;
    double dev = 0.0, sq = 0.0;
    for (long e = t; e < inner; e += 256) {
        double v[SSD_MAX_AGENTS];
#pragma unroll
        for (int i = 0; i < SSD_MAX_AGENTS; ++i)
            if (i < copies) v[i] = (double)base[i * inner + e];
        double s = v[0];
#pragma unroll
        for (int i = 1; i < SSD_MAX_AGENTS; ++i)
            if (i < copies) s += v[i];
        const double m = s / (double)copies;
#pragma unroll
        for (int i = 0; i < SSD_MAX_AGENTS; ++i)
            if (i < copies) {
                const double d = v[i] - m;
                dev += d * d;
                sq += v[i] * v[i];
            }
    }
    red[0][t] = dev;
    red[1][t] = sq;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] += red[0][t + s];
            red[1][t] += red[1][t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[2 * (size_t)blockIdx.x] = red[0][0];
        out[2 * (size_t)blockIdx.x + 1] = red[1][0];
    }
}

void launch_tie_agent_grads(float* flat, const int64_t* jobs_dev, int n_jobs, long max_inner, hipStream_t s) {
    long bx = (max_inner + kTieThreads - 1) / kTieThreads;
    if (bx > kTieMaxBlocksX) bx = kTieMaxBlocksX;
    hipLaunchKernelGGL(k_tie_agent_grads, dim3((unsigned)bx, (unsigned)n_jobs), dim3(kTieThreads), 0, s, flat, jobs_dev);
}

void launch_agent_spread(const int64_t* jobs_dev, int n_jobs, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_agent_spread, dim3((unsigned)n_jobs), dim3(256), 0, s, jobs_dev, out);
}

}  // namespace ssd
