// rotate-yolov3_amd/csrc/optim.hip -- one launch for the whole optimizer step, SGD or Adam (train.py:70-83 builds
// torch.optim.SGD with momentum + nesterov, or torch.optim.Adam with --adam; weight decay on the conv weights only; ATen runs
// either as a chain of foreach kernels over the parameter tensors: about 30 launches for SGD, 60 for Adam).
// SGD.
// Same fp32 arithmetic, same order (built without fp contraction):
//   d = g (+ wd * p);  buf = first ? d : momentum * buf + d;  d = nesterov ? d + momentum * buf : buf;  p -= lr * d
// Optional per-group gradient scale (hparam slot 3; 0 = none): data-parallel training passes 1/world here instead of dividing
// the 250 MB all-reduced gradient in a separate pass (dist.py).
// Adam: torch.optim.Adam's multi-tensor step (amsgrad = maximize = False, L2 weight decay), operator by operator in fp32:
//   d = g (* gs) (+ wd * p)                                   _foreach_add(alpha = wd)
//   m = m + (1-b1) * (d - m)                                  _foreach_lerp_   (weight >= 0.5: d - (d - m) * (1 - (1-b1)), as ATen)
//   v = v * b2;  v = v + ((1-b2) * d) * d                     _foreach_mul_, _foreach_addcmul_ (value * t1 first: finite where d * d is not)
//   den = sqrt(v) / bc2_sqrt + eps;  p = p + step_size * (m / den)        _foreach_sqrt, div_, add_, addcdiv_
// IEEE sqrt and divide, no contraction.  The scalars are computed on the host in doubles and arrive as fp32, as ATen's scalar
// arguments do; one row of 8 per (param group, step count).  Memory bound: 4 loads + 3 stores per element, 16 bytes per lane where
// the four pointers of a tensor allow it, the same per-element function on either path (identical bits).  No LDS, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ryolo.h"

namespace {

__global__ void __launch_bounds__(256) sgd_batch_kernel(const ryolo_sgd_job *__restrict__ jobs, int njobs,
                                                        const float *__restrict__ hp /* [groups][4] lr, momentum, wd, grad scale */,
                                                        int nesterov) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block_begin <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ryolo_sgd_job j = jobs[lo];
    const float lr = hp[j.group * 4 + 0], mom = hp[j.group * 4 + 1], wd = hp[j.group * 4 + 2], gs = hp[j.group * 4 + 3];
    float *__restrict__ p = (float *)j.p;
    const float *__restrict__ g = (const float *)j.g;
    float *__restrict__ buf = (float *)j.buf;
    const long long nblk = j.block_end - j.block_begin;
    for (long long i = (long long)((int)blockIdx.x - j.block_begin) * 256 + threadIdx.x; i < j.n; i += nblk * 256) {
        const float pv = p[i];
        float d = g[i];
        if (gs != 0.f) d = d * gs;
        if (wd != 0.f) d = d + wd * pv;
        if (mom != 0.f) {
            const float b = j.first ? d : mom * buf[i] + d;
            buf[i] = b;
            d = nesterov ? d + mom * b : b;
        }
        p[i] = pv - lr * d;
    }
}

struct AdamRow {
    float step_size, bc2_sqrt, omb1, b2, omb2, eps, wd, gs;
};

__device__ __forceinline__ void adam_elem(float &p, float g, float &m, float &v, const AdamRow &r) {
    float d = g;
    if (r.gs != 0.f) d = d * r.gs;
    if (r.wd != 0.f) d = d + r.wd * p;
    m = r.omb1 < 0.5f ? m + r.omb1 * (d - m) : d - (d - m) * (1.f - r.omb1);
    v = v * r.b2;
    v = v + (r.omb2 * d) * d;
    const float den = sqrtf(v) / r.bc2_sqrt + r.eps;
    p = p + r.step_size * (m / den);
}

__global__ void __launch_bounds__(256) adam_batch_kernel(const ryolo_adam_job *__restrict__ jobs, int njobs,
                                                         const float *__restrict__ rows /* [rows][8], see AdamRow */) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block_begin <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ryolo_adam_job j = jobs[lo];
    const float *rr = rows + (long long)j.row * 8;
    const AdamRow r = {rr[0], rr[1], rr[2], rr[3], rr[4], rr[5], rr[6], rr[7]};
    float *__restrict__ p = (float *)j.p;
    const float *__restrict__ g = (const float *)j.g;
    float *__restrict__ m = (float *)j.m;
    float *__restrict__ v = (float *)j.v;
    const long long stride = (long long)(j.block_end - j.block_begin) * 256;
    const long long first = (long long)((int)blockIdx.x - j.block_begin) * 256 + threadIdx.x;
    long long scalar_from = first;          // the 4-byte path: everything, or the (n & 3)-element tail behind the 16-byte path
    if ((((uintptr_t)j.p | (uintptr_t)j.g | (uintptr_t)j.m | (uintptr_t)j.v) & 15) == 0) {
        const long long n4 = j.n >> 2;
        for (long long i = first; i < n4; i += stride) {
            float4 pv = ((const float4 *)p)[i], mv = ((const float4 *)m)[i], vv = ((const float4 *)v)[i];
            const float4 gv = ((const float4 *)g)[i];
            adam_elem(pv.x, gv.x, mv.x, vv.x, r);
            adam_elem(pv.y, gv.y, mv.y, vv.y, r);
            adam_elem(pv.z, gv.z, mv.z, vv.z, r);
            adam_elem(pv.w, gv.w, mv.w, vv.w, r);
            ((float4 *)p)[i] = pv;
            ((float4 *)m)[i] = mv;
            ((float4 *)v)[i] = vv;
        }
        scalar_from = n4 * 4 + first;
    }
    for (long long i = scalar_from; i < j.n; i += stride) {
        float pv = p[i], mv = m[i], vv = v[i];
        adam_elem(pv, g[i], mv, vv, r);
        p[i] = pv;
        m[i] = mv;
        v[i] = vv;
    }
}

}  // namespace

extern "C" {

int ryolo_sgd_step(const ryolo_sgd_job *device_jobs, int njobs, int total_blocks, const float *group_hparams, int nesterov,
                   void *stream) {
    if (!device_jobs || njobs <= 0 || total_blocks <= 0 || !group_hparams) return RYOLO_EINVAL;
    hipLaunchKernelGGL(sgd_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, device_jobs, njobs,
                       group_hparams, nesterov);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

int ryolo_adam_step(const ryolo_adam_job *device_jobs, int njobs, int total_blocks, const float *rows, void *stream) {
    if (!device_jobs || njobs <= 0 || total_blocks <= 0 || !rows) return RYOLO_EINVAL;
    hipLaunchKernelGGL(adam_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, device_jobs, njobs, rows);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

}  // extern "C"
