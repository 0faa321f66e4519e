// detpost.hip -- what the reference's detect.py does to every detection in Python after the NMS, one launch per batch each:
//
// ryolo_det_rescale   scale_coords(img.shape[2:], det[:, :4], im0.shape).round() (utils/utils.py:181-189) on the flat rows of a batch:
//                     row r belongs to image b with det_off[b] <= r < det_off[b + 1]; geom[b] = (gain, pad_x, pad_y) in fp32;
//                     columns 0, 1 become rintf((v - pad) / gain), columns 2, 3 rintf(v / gain), columns 4..7 stay.  The division is a
//                     true fp32 division (the unit is built with -ffp-contract=off and IEEE divide).
// ryolo_det_quads     xywha2icdar (utils/ICDAR/icdar_utils.py:105-135) per row, in fp64: the corners (xmin, ymin), (xmin, ymax),
//                     (xmax, ymax), (xmax, ymin) of the upright box turned by alpha = cos(-a), beta = sin(-a) about the centre --
//                         X = tx * alpha + ty * beta + ((1 - alpha) * cx - beta * cy),   Y = tx * -beta + ty * alpha + (beta * cx + (1 - alpha) * cy)
//                     -- then order_points: stable sort by X (ties by corner index); the two left-most, stably by Y, are tl, bl; of the two
//                     right-most the one farther from tl (squared distance) is br, on a tie the later one; the output row is
//                     tl, tr, br, bl with every coordinate truncated toward zero to int32.
// ryolo_det_corners   get_rotated_coors (utils/utils.py:702-725) per row: the same four turned corners in fp64, kept in THAT order
//                     (corner 0 is where the drawn label is anchored, and order_points can return a sequence that is no cycle on ties)
//                     and truncated toward zero to int32 -- the outline csrc/draw.hip draws.
// One thread per row, no workspace, no atomics.  tests/detect_reference.py restates the first two, tests/draw_reference.py the third.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ryolo.h"

namespace {

__global__ __launch_bounds__(256) void det_rescale_kernel(float *__restrict__ det, int M, const int *__restrict__ det_off, int bs,
                                                          const float *__restrict__ geom) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    int lo = 0, hi = bs;                 // the image b with det_off[b] <= r < det_off[b + 1]: the last b with det_off[b] <= r
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (det_off[mid] <= r) lo = mid; else hi = mid;
    }
    const float gain = geom[3 * lo], px = geom[3 * lo + 1], py = geom[3 * lo + 2];
    float4 v = *(float4 *)(det + (size_t)r * 8);
    v.x = rintf((v.x - px) / gain);
    v.y = rintf((v.y - py) / gain);
    v.z = rintf(v.z / gain);
    v.w = rintf(v.w / gain);
    *(float4 *)(det + (size_t)r * 8) = v;
}

__global__ __launch_bounds__(256) void det_quads_kernel(const float *__restrict__ det, int M, int *__restrict__ quad) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    const float4 v = *(const float4 *)(det + (size_t)r * 8);
    const double cx = v.x, cy = v.y, w = v.z, h = v.w, a = det[(size_t)r * 8 + 4];
    const double alpha = cos(-a), beta = sin(-a);
    const double r02 = (1 - alpha) * cx - beta * cy, r12 = beta * cx + (1 - alpha) * cy;
    const double tx[4] = {cx - w * 0.5, cx - w * 0.5, cx + w * 0.5, cx + w * 0.5};
    const double ty[4] = {cy - h * 0.5, cy + h * 0.5, cy + h * 0.5, cy - h * 0.5};
    double X[4], Y[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        X[k] = tx[k] * alpha + ty[k] * beta + r02;
        Y[k] = tx[k] * -beta + ty[k] * alpha + r12;
    }
    int o[4] = {0, 1, 2, 3};             // stable insertion sort by X
#pragma unroll
    for (int i = 1; i < 4; i++) {
#pragma unroll
        for (int j = i; j > 0; j--) {
            if (X[o[j]] < X[o[j - 1]]) { const int t = o[j]; o[j] = o[j - 1]; o[j - 1] = t; }
        }
    }
    int tl = o[0], bl = o[1];
    if (Y[bl] < Y[tl]) { const int t = tl; tl = bl; bl = t; }
    const double d0 = (X[o[2]] - X[tl]) * (X[o[2]] - X[tl]) + (Y[o[2]] - Y[tl]) * (Y[o[2]] - Y[tl]);
    const double d1 = (X[o[3]] - X[tl]) * (X[o[3]] - X[tl]) + (Y[o[3]] - Y[tl]) * (Y[o[3]] - Y[tl]);
    int br = o[3], tr = o[2];
    if (d0 > d1) { br = o[2]; tr = o[3]; }
    int4 q0, q1;
    q0.x = (int)X[tl]; q0.y = (int)Y[tl]; q0.z = (int)X[tr]; q0.w = (int)Y[tr];
    q1.x = (int)X[br]; q1.y = (int)Y[br]; q1.z = (int)X[bl]; q1.w = (int)Y[bl];
    *(int4 *)(quad + (size_t)r * 8) = q0;
    *(int4 *)(quad + (size_t)r * 8 + 4) = q1;
}

__global__ __launch_bounds__(256) void det_corners_kernel(const float *__restrict__ det, int M, int *__restrict__ quad) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    const float4 v = *(const float4 *)(det + (size_t)r * 8);
    const double cx = v.x, cy = v.y, w = v.z, h = v.w, a = det[(size_t)r * 8 + 4];
    const double alpha = cos(-a), beta = sin(-a);
    const double r02 = (1 - alpha) * cx - beta * cy, r12 = beta * cx + (1 - alpha) * cy;
    const double tx[4] = {cx - w * 0.5, cx - w * 0.5, cx + w * 0.5, cx + w * 0.5};
    const double ty[4] = {cy - h * 0.5, cy + h * 0.5, cy + h * 0.5, cy - h * 0.5};
    int q[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {        // the corners stay in get_rotated_coors' order: no order_points
        q[2 * k] = (int)(tx[k] * alpha + ty[k] * beta + r02);
        q[2 * k + 1] = (int)(tx[k] * -beta + ty[k] * alpha + r12);
    }
    *(int4 *)(quad + (size_t)r * 8) = make_int4(q[0], q[1], q[2], q[3]);
    *(int4 *)(quad + (size_t)r * 8 + 4) = make_int4(q[4], q[5], q[6], q[7]);
}

}  // namespace

extern "C" {

int ryolo_det_rescale(float *det, int M, const int *det_off, int bs, const float *geom, void *stream) {
    if (M < 0 || bs < 1) return RYOLO_EINVAL;
    if (M == 0) return RYOLO_OK;
    if (!det || !det_off || !geom || ((uintptr_t)det & 15)) return RYOLO_EINVAL;
    hipLaunchKernelGGL(det_rescale_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, det, M, det_off, bs, geom);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

int ryolo_det_quads(const float *det, int M, int *quad, void *stream) {
    if (M < 0) return RYOLO_EINVAL;
    if (M == 0) return RYOLO_OK;
    if (!det || !quad || ((uintptr_t)det & 15) || ((uintptr_t)quad & 15)) return RYOLO_EINVAL;
    hipLaunchKernelGGL(det_quads_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, det, M, quad);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

int ryolo_det_corners(const float *det, int M, int *quad, void *stream) {
    if (M < 0) return RYOLO_EINVAL;
    if (M == 0) return RYOLO_OK;
    if (!det || !quad || ((uintptr_t)det & 15) || ((uintptr_t)quad & 15)) return RYOLO_EINVAL;
    hipLaunchKernelGGL(det_corners_kernel, dim3((M + 255) / 256), dim3(256), 0, (hipStream_t)stream, det, M, quad);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

}  // extern "C"
