// rotate-yolov3_amd/csrc/skewiou.hip -- rotated IoU of the EVALUATION path: the value the reference's skew_bbox_iou returns
// (utils/utils.py:290-320 -> get_rotated_coors :702-725 -> skewiou :663-699, shapely polygon intersection in fp64), which
// test.py:146 thresholds to mark a prediction correct.  It is NOT the arithmetic of the native NMS kernel (rnms.hip keeps
// that one bit for bit, including its behaviour on coincident boxes, where it can report 1/3 for IoU(A, A)): here the four
// corners are computed in fp64 with get_rotated_coors' rotation matrix (OpenCV getRotationMatrix2D of angle -a about the
// centre) and the intersection of the two convex quadrilaterals is an fp64 Sutherland-Hodgman clip + shoelace areas --
// the exact geometry, to fp64 rounding.  One pair per lane; the polygon (<= 8 vertices) lives in registers / scratch-free
// local arrays with fully unrolled loops.  Replaces the per-pair Python + shapely loop by one launch per image.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ryolo.h"

namespace {

struct Quad { double x[4], y[4]; };

__device__ __forceinline__ void corners(const float *b, Quad &q) {
    // get_rotated_coors: (xmin,ymin) (xmin,ymax) (xmax,ymax) (xmax,ymin) mapped by R = getRotationMatrix2D((cx,cy), -a*180/pi, 1)
    //   R = [[al, be, (1-al)cx - be*cy], [-be, al, be*cx + (1-al)cy]], al = cos(-a), be = sin(-a)
    const double cx = b[0], cy = b[1], w = b[2], h = b[3], a = b[4];
    const double al = cos(-a), be = sin(-a);
    const double r02 = (1.0 - al) * cx - be * cy, r12 = be * cx + (1.0 - al) * cy;
    const double xs[2] = {cx - w * 0.5, cx + w * 0.5}, ys[2] = {cy - h * 0.5, cy + h * 0.5};
    const int ix[4] = {0, 0, 1, 1}, iy[4] = {0, 1, 1, 0};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double tx = xs[ix[k]], ty = ys[iy[k]];
        q.x[k] = tx * al + ty * be + r02;
        q.y[k] = -tx * be + ty * al + r12;
    }
}

__device__ __forceinline__ double quad_area2(const Quad &q) {   // twice the signed area
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int n = (k + 1) & 3;
        s += q.x[k] * q.y[n] - q.x[n] * q.y[k];
    }
    return s;
}

// Everything skew_iou computes from ONE box: its corners, twice its area, and the swap that makes the quadrilateral counter-clockwise.
__device__ __forceinline__ double oriented_quad(const float *b, Quad &q) {
    corners(b, q);
    double a = quad_area2(q);
    if (a < 0) {       // make it counter-clockwise
        double t;
        t = q.x[1]; q.x[1] = q.x[3]; q.x[3] = t;
        t = q.y[1]; q.y[1] = q.y[3]; q.y[3] = t;
        a = -a;
    }
    return a;
}

// The per-pair half of skew_iou on two oriented quadrilaterals and their twice-areas.
__device__ double clip_iou(const Quad &p, double a1, const Quad &c, double a2) {
    if (a1 == 0.0 || a2 == 0.0) return 0.0;                 // skewiou: "if poly1.area == 0 or poly2.area == 0: return 0"
    // Sutherland-Hodgman: clip p by the four half planes of c.  A convex quadrilateral clipped by 4 lines has <= 8 vertices.
    double px[8], py[8], qx[8], qy[8];
    int n = 4;
#pragma unroll
    for (int k = 0; k < 4; k++) { px[k] = p.x[k]; py[k] = p.y[k]; }
    for (int e = 0; e < 4 && n > 0; e++) {
        const double ax = c.x[e], ay = c.y[e];
        const double ex = c.x[(e + 1) & 3] - ax, ey = c.y[(e + 1) & 3] - ay;
        int m = 0;
        for (int j = 0; j < n; j++) {
            const int j2 = j + 1 == n ? 0 : j + 1;
            const double sp = ex * (py[j] - ay) - ey * (px[j] - ax);
            const double sq = ex * (py[j2] - ay) - ey * (px[j2] - ax);
            if (sp >= 0.0 && m < 8) { qx[m] = px[j]; qy[m] = py[j]; m++; }
            if (((sp > 0.0 && sq < 0.0) || (sp < 0.0 && sq > 0.0)) && m < 8) {
                const double t = sp / (sp - sq);
                qx[m] = px[j] + t * (px[j2] - px[j]);
                qy[m] = py[j] + t * (py[j2] - py[j]);
                m++;
            }
        }
        n = m;
        for (int j = 0; j < n; j++) { px[j] = qx[j]; py[j] = qy[j]; }
    }
    double inter2 = 0.0;
    for (int j = 0; j < n; j++) {
        const int j2 = j + 1 == n ? 0 : j + 1;
        inter2 += px[j] * py[j2] - px[j2] * py[j];
    }
    inter2 = fabs(inter2);
    const double uni2 = a1 + a2 - inter2;
    if (uni2 == 0.0) return 0.0;
    return inter2 / uni2;
}

__device__ double skew_iou(const float *b1, const float *b2) {
    Quad p, c;
    const double a1 = oriented_quad(b1, p), a2 = oriented_quad(b2, c);
    return clip_iou(p, a1, c, a2);
}

__global__ void skew_iou_pairs_kernel(const float *b1, int s1, const float *b2, int s2, int n, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)skew_iou(b1 + (size_t)i * s1, b2 + (size_t)i * s2);
}

__global__ void skew_iou_matrix_kernel(const float *b1, int n1, int s1, const float *b2, int n2, int s2, float *out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j < n2) out[(size_t)i * n2 + j] = (float)skew_iou(b1 + (size_t)i * s1, b2 + (size_t)j * s2);
}

// ---- mAP matching of a whole batch (ryolo_eval_match): the greedy loop of the reference's test.py:121-151 without its serial walk.
// For prediction i of an image, best(i) = the same-class label of that image with the largest fp32 IoU (lowest label on ties, what
// torch.max(0) returns) and i CLAIMS best(i) when that IoU > thres in fp32.  A label is marked detected only by a correct prediction
// whose best it is, so the first claimant of a label always finds it free and every later one finds it taken:
//     correct[i]  <=>  i claims best(i) and no smaller index of its image claims the same label.
// Three launches: labels -> oriented corners (once per label, not per pair), predictions -> best + atomicMin of the claimant's index,
// predictions -> compare.  Integer min does not depend on the order of the atomics: the result is deterministic.

struct LabelRec {            // one label in the workspace: what oriented_quad gives for it, and its bounding circle
    Quad q;
    double area2, cx, cy, r;
};

constexpr int EM_THREADS = 64;          // one wave per workgroup: predictions of one image share their label loads
constexpr int EM_LDS_OFFSETS = 256;     // image offsets kept in LDS up to this many entries; longer tables are bisected in global memory

__device__ __forceinline__ double circle_radius(const float *b) {
    const double w = b[2], h = b[3];
    return 0.5 * sqrt(w * w + h * h);
}

__global__ void eval_match_prep_kernel(const float *lab, int lab_stride, int n_lab, LabelRec *rec, int *first) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_lab) return;
    const float *b = lab + (size_t)g * lab_stride + 1;      // (cls, x, y, w, h, a): the box starts at column 1
    LabelRec r;
    r.area2 = oriented_quad(b, r.q);
    r.cx = b[0];
    r.cy = b[1];
    r.r = circle_radius(b);
    rec[g] = r;
    first[g] = 0x7fffffff;
}

__global__ void __launch_bounds__(EM_THREADS)
eval_match_best_kernel(const float *det, int det_stride, const int *det_off, const float *lab, int lab_stride, const int *lab_off,
                       int n_img, int n_det, int n_lab, float thres, const LabelRec *rec, int *first, int *best) {
    __shared__ int s_off[EM_LDS_OFFSETS];
    const int *off = det_off;
    if (n_img + 1 <= EM_LDS_OFFSETS) {
        for (int k = threadIdx.x; k <= n_img; k += EM_THREADS) s_off[k] = det_off[k];
        __syncthreads();
        off = s_off;
    }
    const int i = blockIdx.x * EM_THREADS + threadIdx.x;
    if (i >= n_det) return;
    int lo = 0, hi = n_img;             // the image of row i: the last im with off[im] <= i (empty images share an offset with their successor)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    int g0 = lab_off[lo], g1 = lab_off[lo + 1];
    g0 = g0 < 0 ? 0 : g0;               // a broken offset table reads no memory outside the label rows
    g1 = g1 > n_lab ? n_lab : g1;
    const float *b = det + (size_t)i * det_stride;
    const float cls = b[7];
    Quad p;
    const double a1 = oriented_quad(b, p);
    const double pcx = b[0], pcy = b[1], pr = circle_radius(b);
    float bv = -INFINITY;
    int bg = -1;
    bool nan_seen = false;
    for (int g = g0; g < g1; g++) {
        if (!(lab[(size_t)g * lab_stride] == cls)) continue;
        const LabelRec *l = rec + g;
        // Bounding-circle reject.  Every corner lies within r (1 + 4 ulp) + 4 ulp (|cx| + |cy|) of its centre in fp64, and a vertex that
        // survives all four clip stages lies within such rounding of BOTH quadrilaterals; with the centres further apart than the radii
        // plus 2^-20 of (radii + centre coordinates) -- ten orders of magnitude above that rounding -- no vertex survives, and the clip
        // returns fabs(0) / (a1 + a2) = +0.0 (or the zero-area 0.0): exactly the value skipped here.  Non-finite operands fail the
        // comparison and take the clip.  A skipped 0 never wins the strict maximum over a positive IoU and never exceeds thres >= 0.
        const double dx = pcx - l->cx, dy = pcy - l->cy, d2 = dx * dx + dy * dy;
        const double s = pr + l->r, lim = s + 0x1p-20 * (s + fabs(pcx) + fabs(pcy) + fabs(l->cx) + fabs(l->cy));
        float v = 0.0f;
        if (!(d2 > lim * lim && d2 < (double)INFINITY)) v = (float)clip_iou(p, a1, l->q, l->area2);
        if (v != v) nan_seen = true;    // torch.max returns a NaN maximum, and NaN > thres is false: such a prediction claims nothing
        if (v > bv) { bv = v; bg = g; }
    }
    const bool claims = bg >= 0 && !nan_seen && bv > thres;
    best[i] = claims ? bg : -1;
    if (claims) atomicMin(first + bg, i);
}

// best == NULL: a batch without labels, nothing is correct
__global__ void eval_match_resolve_kernel(const int *best, const int *first, int n_det, uint8_t *correct, int32_t *matched) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_det) return;
    const int g = best ? best[i] : -1;
    const bool ok = g >= 0 && first[g] == i;
    correct[i] = ok ? 1 : 0;
    if (matched) matched[i] = ok ? g : -1;
}

// workspace: LabelRec[n_lab] | int first[n_lab] | int best[n_det]
inline size_t em_rec_bytes(int n_lab) { return (size_t)n_lab * sizeof(LabelRec); }

}  // namespace

extern "C" {

int ryolo_skew_iou_pairs(const float *b1, int stride1, const float *b2, int stride2, int n, float *out, void *stream_) {
    if (n < 0) return RYOLO_EINVAL;
    if (n == 0) return RYOLO_OK;
    if (!b1 || !b2 || !out || stride1 < 5 || stride2 < 5) return RYOLO_EINVAL;
    hipLaunchKernelGGL(skew_iou_pairs_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream_, b1, stride1, b2, stride2,
                       n, out);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

int ryolo_skew_iou_matrix(const float *b1, int n1, int stride1, const float *b2, int n2, int stride2, float *out, void *stream_) {
    if (n1 < 0 || n2 < 0) return RYOLO_EINVAL;
    if (n1 == 0 || n2 == 0) return RYOLO_OK;
    if (!b1 || !b2 || !out || stride1 < 5 || stride2 < 5 || n1 > 65535) return RYOLO_EINVAL;
    hipLaunchKernelGGL(skew_iou_matrix_kernel, dim3((n2 + 127) / 128, n1), dim3(128), 0, (hipStream_t)stream_, b1, n1, stride1, b2,
                       n2, stride2, out);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

size_t ryolo_eval_match_workspace_bytes(int n_det, int n_lab) {
    if (n_det < 0 || n_lab < 0) return 0;
    return em_rec_bytes(n_lab) + (size_t)n_lab * sizeof(int) + (size_t)n_det * sizeof(int);
}

int ryolo_eval_match(const float *det, int det_stride, const int32_t *det_off, const float *lab, int lab_stride, const int32_t *lab_off,
                     int n_img, int n_det, int n_lab, float iou_thres, uint8_t *correct, int32_t *matched, void *ws, size_t ws_bytes,
                     void *stream_) {
    if (n_img < 0 || n_det < 0 || n_lab < 0 || det_stride < 8 || lab_stride < 6) return RYOLO_EINVAL;
    if (!(iou_thres >= 0.0f && iou_thres < 1.0f)) return RYOLO_EINVAL;                   // NaN fails both comparisons
    if (ws_bytes < ryolo_eval_match_workspace_bytes(n_det, n_lab)) return RYOLO_EINVAL;
    if (n_det > 0 && (!det || !det_off || !correct || n_img == 0)) return RYOLO_EINVAL;
    if (n_det > 0 && n_lab > 0 && (!lab || !lab_off || !ws || ((uintptr_t)ws & 7))) return RYOLO_EINVAL;
    if (n_det == 0) return RYOLO_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 det_grid((n_det + EM_THREADS - 1) / EM_THREADS), block(EM_THREADS);
    if (n_lab == 0) {
        hipLaunchKernelGGL(eval_match_resolve_kernel, det_grid, block, 0, stream, (const int *)nullptr, (const int *)nullptr, n_det, correct,
                           matched);
        return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
    }
    LabelRec *rec = (LabelRec *)ws;
    int *first = (int *)((char *)ws + em_rec_bytes(n_lab)), *best = first + n_lab;
    hipLaunchKernelGGL(eval_match_prep_kernel, dim3((n_lab + EM_THREADS - 1) / EM_THREADS), block, 0, stream, lab, lab_stride, n_lab, rec,
                       first);
    if (hipGetLastError() != hipSuccess) return RYOLO_ELAUNCH;
    hipLaunchKernelGGL(eval_match_best_kernel, det_grid, block, 0, stream, det, det_stride, det_off, lab, lab_stride, lab_off, n_img, n_det,
                       n_lab, iou_thres, (const LabelRec *)rec, first, best);
    if (hipGetLastError() != hipSuccess) return RYOLO_ELAUNCH;
    hipLaunchKernelGGL(eval_match_resolve_kernel, det_grid, block, 0, stream, (const int *)best, (const int *)first, n_det, correct, matched);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

}  // extern "C"
