/* ssd_hip_tie.h -- the entry points of libssd_hip.so for heads shared across agents (config key share_heads): the gradients of the n
 * per-agent copies of a tensor summed into one and written back to all copies, and the spread of the copies around their mean.  A
 * companion of ssd_hip.h (types, status codes, ssd_last_error, the ABI version, SSD_ADAM_MAX_JOBS, SSD_MAX_AGENTS: all there);
 * mirrored by homophily_marl_amd/abi.py: TIE_SIGNATURES.  Both functions return an ssd_status.
 *
 * A job table is n_jobs triples of int64, given twice with the same contents: jobs_host (host memory, read by the entry point, which
 * checks it) and jobs_dev (device memory, read by the launch; it must stay alive until the launch -- and every replay of a graph that
 * captured it -- has run).  n_jobs = 0 returns SSD_OK without a launch (the tables may then be NULL).
 *
 * ssd_tie_agent_grads(flat, total, jobs_host, jobs_dev, n_jobs, stream)
 *   flat f32 [total]: the learner's flat gradient buffer (the one ssd_clip_adam_step reads).  Job = {offset, copies, inner}, in elements:
 *   copy i of the tensor is flat[offset + i * inner .. offset + (i + 1) * inner).  For every element e < inner
 *       s = fl(...fl(fl(g_0[e] + g_1[e]) + g_2[e])... + g_{copies-1}[e])      f32, ascending i, one rounding per add
 *   is written to all copies.  It is the sum, not the mean: the gradient of the same loss with respect to ONE shared parameter.  One
 *   launch, no atomics, no scratch memory: a run equals its restatement in plain loops to the bit (NaN payloads aside).  Nothing
 *   outside the jobs' extents is read or written.  Only 4-byte alignment is needed: offsets land on every residue; a job whose inner is
 *   a multiple of 4 moves 16 bytes per access between its first and last 16-byte boundary.
 *   SSD_ERR_INVALID, before any launch, from the host table: a NULL flat, jobs_host or jobs_dev; n_jobs outside 0 .. SSD_ADAM_MAX_JOBS;
 *   total outside 1 .. 2^31 - 1; copies outside 2 .. SSD_MAX_AGENTS; inner < 1; offset < 0; an extent offset + copies * inner past total;
 *   jobs that overlap or do not ascend (offset below the previous job's end); a flat pointer that is not 4-byte aligned.
 *
 * ssd_agent_spread(jobs_host, jobs_dev, n_jobs, out, stream)
 *   Job = {address, copies, inner}: f32 copies at address + 4 * i * inner bytes (the parameters themselves).  out f64 [n_jobs][2]:
 *       out[j][0] = sum_e sum_i (t_i[e] - m[e])^2,   out[j][1] = sum_e sum_i t_i[e]^2,   m[e] = (sum_i t_i[e]) / copies
 *   All arithmetic is f64 on the f32 inputs; sums over i ascend.  One workgroup of 256 threads per job: thread t adds its elements
 *   t, t + 256, ... in rising order, then the 256 accumulators fold by halves (128, 64, ... 1): the same bits run to run.  Copies that
 *   are equal to the bit give out[j][0] = 0 exactly (copies * t is exact in f64 and divides back to t).  Not meant for a captured graph's
 *   hot path: the learner launches it at its log interval.
 *   SSD_ERR_INVALID, before any launch: a NULL jobs_host, jobs_dev or out; n_jobs outside 0 .. SSD_ADAM_MAX_JOBS; an address that is 0 or
 *   not 4-byte aligned; copies outside 2 .. SSD_MAX_AGENTS; inner outside 1 .. 2^31 - 1 over copies; an out that is not 8-byte aligned. */
#ifndef SSD_HIP_TIE_H
#define SSD_HIP_TIE_H

#include "ssd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int ssd_tie_agent_grads(float* flat, int64_t total, const int64_t* jobs_host, const int64_t* jobs_dev, int32_t n_jobs, void* stream);
int ssd_agent_spread(const int64_t* jobs_host, const int64_t* jobs_dev, int32_t n_jobs, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_TIE_H */
