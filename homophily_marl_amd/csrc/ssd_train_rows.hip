// ssd_train_rows.hip -- fc1's input rows of the learner's time-batched evaluation, assembled where fc1 reads them (include/ssd_hip_train.h:
// ssd_fc1_rows_fwd / _bwd).
//
// Reference: the controller concatenates the encoder's features with the non-visual input columns per (episode, timestep, agent)
// (homophily_controller.py:127-184), and the incentive head's fc1 reads those inputs next to the one-hot action
// (homophily_agent.py:179-182).  The learner evaluates the per-agent layers on set-major, time-major rows [n, T * B, .], so the two
// concatenations and the transposition between them were three copy launches per net and five more launches on the way back
// (gradient add, slices, transposition).  Here ONE launch writes the rows of both fc1 layers of the live and of the target net from
// the pieces where they lie, and one launch returns the features' gradient: the sum of the two layers' input gradients, transposed
// back.  Pure data movement plus that one addition of two values: every number is the one the tensor operations produced.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ssd_hip.h"
#include "ssd_device.h"

namespace ssd {

// One thread per (net, agent i, row tb = t * B + b, column c of the wide rows): column c < F0 comes from feat[(b * T + t) * n + i][c],
// c < F0 + F1 from tail (same row), the rest from act[i][tb] -- written to x_inc[net][i][tb][c] and, for c < F0 + F1, to x_env.
__global__ __launch_bounds__(256) void k_fc1_rows(const float* __restrict__ feat_a, const float* __restrict__ feat_b, const float* __restrict__ tail,
                                                  const float* __restrict__ act, float* __restrict__ xe_a, float* __restrict__ xi_a,
                                                  float* __restrict__ xe_b, float* __restrict__ xi_b, int B, int T, int n, int F0, int F1, int A, int nets) {
    const int W = F0 + F1 + A, We = F0 + F1;
    const long TB = (long)T * B, per_net = (long)n * TB * W, total = per_net * nets;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int net = (int)(idx / per_net);
        const long e = idx - net * per_net, row = e / W;               // row = i * TB + tb
        const int c = (int)(e - row * W), i = (int)(row / TB);
        const long tb = row - i * TB;
        const int t = (int)(tb / B), b = (int)(tb - (long)t * B);
        const long src = ((long)b * T + t) * n + i;
        float v;
        if (c < F0) v = (net ? feat_b : feat_a)[src * F0 + c];
        else if (c < We) v = tail[src * F1 + (c - F0)];
        else v = act[row * A + (c - We)];
        (net ? xi_b : xi_a)[row * W + c] = v;
        if (c < We) (net ? xe_b : xe_a)[row * We + c] = v;
    }
}

// d_feat[(b * T + t) * n + i][c] = dxe[i][t * B + b][c] + dxi[i][t * B + b][c] for c < F0: one thread per element of d_feat, whose rows
// lie ld floats apart (ld >= F0: the caller may hand out the leading columns of wider rows, as the slice of a concatenation's gradient is)
__global__ __launch_bounds__(256) void k_fc1_rows_bwd(const float* __restrict__ dxe, const float* __restrict__ dxi, float* __restrict__ d_feat, int B, int T,
                                                      int n, int F0, int F1, int A, int ld) {
    const int W = F0 + F1 + A, We = F0 + F1;
    const long TB = (long)T * B, total = (long)n * TB * F0;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long src = idx / F0;                                     // (b * T + t) * n + i
        const int c = (int)(idx - src * F0), i = (int)(src % n);
        const long bt = src / n;
        const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
        const long row = (long)i * TB + (long)t * B + b;
        d_feat[src * ld + c] = dxe[row * We + c] + dxi[row * W + c];
    }
}

static int rows_grid(long total) {
    const long b = (total + 255) / 256;
    return (int)(b > 16384 ? 16384 : b);
}

void launch_fc1_rows(const float* feat_a, const float* feat_b, const float* tail, const float* act, float* xe_a, float* xi_a, float* xe_b, float* xi_b, int B,
                     int T, int n, int F0, int F1, int A, hipStream_t s) {
    const int nets = feat_b ? 2 : 1;
    const long total = (long)nets * n * T * B * (F0 + F1 + A);
    hipLaunchKernelGGL(k_fc1_rows, dim3(rows_grid(total)), dim3(256), 0, s, feat_a, feat_b, tail, act, xe_a, xi_a, xe_b, xi_b, B, T, n, F0, F1, A, nets);
}

void launch_fc1_rows_bwd(const float* dxe, const float* dxi, float* d_feat, int B, int T, int n, int F0, int F1, int A, int ld, hipStream_t s) {
    const long total = (long)n * T * B * F0;
    hipLaunchKernelGGL(k_fc1_rows_bwd, dim3(rows_grid(total)), dim3(256), 0, s, dxe, dxi, d_feat, B, T, n, F0, F1, A, ld);
}

}  // namespace ssd
