// draw.hip -- ryolo_draw_quads: what the reference's plot_one_box (utils/utils.py:479-490) and plot_images (:514-550) do with
// cv2.polylines / cv2.putText, on the device, with an exact integer definition of our own (cv2 is no dependency and no definition).
//
// The pixels are the image cache's: uint8 RGB HWC, images back to back at img_offset[b] bytes, img_hw[b] = (h, w).  Row r of quad / color /
// lab_* belongs to image b with det_off[b] <= r < det_off[b + 1].  The three bytes of pixel P = (x, y) of image b in dst are color[r*], r*
// the LARGEST row of the image that covers P (a later row paints over an earlier one); without such a row they are those of src.
//
//   outline   corners Q0..Q3 = quad[r], t = thick[b].  Row r covers P when for one of the edges A = Qk, B = Q(k+1 mod 4) the squared distance
//             from P to the closed segment AB satisfies 4 dist^2 <= t^2, decided in integers:  d = B - A, L2 = d.d, u = (P - A).d;
//             u <= 0 or L2 = 0: 4 |P - A|^2 <= t^2;   u >= L2: 4 |P - B|^2 <= t^2;   otherwise c = (P - A) x d and 4 c^2 <= t^2 L2.
//             A thick polyline with round joints and caps of diameter t.  Image sides are at most 16384 and a row with a corner
//             coordinate outside [-16384, 32767] draws nothing (its label neither), so |c| < 2^32 and t^2 L2 < 2^49: the last test is
//             false when 2 |c| >= 2^32 and otherwise both sides fit 64 bits unsigned.  Nothing is rounded.
//   label     lab_rect[r] = (lx, ly, lw, lh): row r covers P when lx <= x < lx + lw, ly <= y < ly + lh and
//             lab_bits[lab_off[r] + (y - ly) lw + (x - lx)] != 0 (one byte per label pixel).  lw <= 0 or lh <= 0: no label.
//
// One launch: a 256-thread workgroup owns a 64 x 64 tile of one image (grid: tiles of max_w x max_h, n_img; tiles outside their image
// leave at once).  It walks the image's rows from the highest down in passes of ROWS_PER_PASS = 256 rows: thread i of a pass takes row
// top - i, culls it against the tile (the quad's bounding box grown by ceil(t / 2), and the label rectangle) and the survivors go to an LDS
// list in descending row order (wave ballots + four wave counts: no atomics).  Each thread owns 4 x 4 pixels, four horizontal runs of four
// (12 bytes); it walks the list and the first entry that covers a pixel settles it.  The passes end when every pixel of the tile is
// settled.  Then each run is read, merged and written: three dwords where its address is 4-byte aligned (images start at any byte offset
// and a pixel is three bytes, so that is decided per run, for src and dst separately), single bytes otherwise and at a ragged right edge.
// A thread reads only the bytes it writes, so dst == src is allowed; then runs without a painted pixel are not written at all.
// No workspace, no allocation, no atomics, one writer per byte, bytes of dst outside the images are not touched.
//
// thick is HOST memory: read and validated in the call and passed on in the kernel arguments (one byte per image, at most
// MAX_IMAGES = 1024), so a captured graph replays the thicknesses it was captured with.  tests/draw_reference.py restates all of this.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ryolo.h"

namespace {

constexpr int TILE = 64;
constexpr int ROWS_PER_PASS = 256;
constexpr int MAX_IMAGES = 1024;
constexpr int MAX_SIDE = 16384;
constexpr int COORD_MIN = -16384, COORD_MAX = 32767;
constexpr unsigned DONE = 1u << 24;

struct Thick { unsigned char t[MAX_IMAGES]; };

struct Entry {
    int q[8];
    int ox0, oy0, ox1, oy1;      // the outline's bounding box grown by ceil(t / 2), inclusive
    int cx0, cy0, cx1, cy1;      // the label rectangle clipped to the image, ends exclusive (empty: no label)
    int lx, ly, lw;
    unsigned color;
    long long loff;
};

__device__ __forceinline__ bool near_point(int ex, int ey, unsigned t2) {
    return 4ull * (unsigned long long)((long long)ex * ex + (long long)ey * ey) <= t2;
}

// 4 dist^2(P, segment AB) <= t^2, exactly
__device__ __forceinline__ bool edge_covers(int px, int py, int ax, int ay, int bx, int by, unsigned t2) {
    const int dx = bx - ax, dy = by - ay, ex = px - ax, ey = py - ay;
    const long long L2 = (long long)dx * dx + (long long)dy * dy;
    const long long u = (long long)ex * dx + (long long)ey * dy;
    if (u <= 0 || L2 == 0) return near_point(ex, ey, t2);
    if (u >= L2) return near_point(px - bx, py - by, t2);
    const long long c = (long long)ex * dy - (long long)ey * dx;
    const unsigned long long c2 = 2ull * (unsigned long long)(c < 0 ? -c : c);
    if (c2 >> 32) return false;
    return c2 * c2 <= (unsigned long long)t2 * (unsigned long long)L2;
}

__global__ __launch_bounds__(256) void draw_quads_kernel(const uint8_t *src, uint8_t *dst, const long long *__restrict__ img_offset,
                                                         const int *__restrict__ img_hw, const int *__restrict__ quad,
                                                         const int *__restrict__ det_off, int M, const uint8_t *__restrict__ color,
                                                         Thick thick, const uint8_t *__restrict__ lab_bits,
                                                         const long long *__restrict__ lab_off, const int *__restrict__ lab_rect) {
    __shared__ Entry list[ROWS_PER_PASS];
    __shared__ int wave_cnt[4];
    const int b = blockIdx.z;
    const int h = img_hw[2 * b], w = img_hw[2 * b + 1];
    const int tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
    if (tx0 >= w || ty0 >= h) return;                    // the whole workgroup: the grid is sized by the largest image
    const int tx1 = min(tx0 + TILE - 1, w - 1), ty1 = min(ty0 + TILE - 1, h - 1);
    const int t = thick.t[b], grow = (t + 1) >> 1;
    const unsigned t2 = (unsigned)(t * t);
    int lo = 0, hi = 0;
    if (M > 0) {
        lo = max(det_off[b], 0);
        hi = min(det_off[b + 1], M);
    }
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int gx = tx0 + (tid & 15) * 4, gy = ty0 + (tid >> 4);          // pixels (gx + p, gy + 16 j), p, j = 0..3

    unsigned res[16];                                    // per pixel: DONE | colour once settled
    int left = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const bool in = gx + p < w && gy + 16 * j < h;
            res[4 * j + p] = in ? 0u : DONE;
            left += in;
        }

    for (int top = hi - 1; top >= lo; top -= ROWS_PER_PASS) {
        // cull: thread i takes row top - i
        const int r = top - tid;
        bool keep = false;
        Entry e;
        if (r >= lo) {
            const int4 q0 = *(const int4 *)(quad + (size_t)r * 8), q1 = *(const int4 *)(quad + (size_t)r * 8 + 4);
            e.q[0] = q0.x; e.q[1] = q0.y; e.q[2] = q0.z; e.q[3] = q0.w;
            e.q[4] = q1.x; e.q[5] = q1.y; e.q[6] = q1.z; e.q[7] = q1.w;
            int mnx = min(min(q0.x, q0.z), min(q1.x, q1.z)), mxx = max(max(q0.x, q0.z), max(q1.x, q1.z));
            int mny = min(min(q0.y, q0.w), min(q1.y, q1.w)), mxy = max(max(q0.y, q0.w), max(q1.y, q1.w));
            if (min(mnx, mny) >= COORD_MIN && max(mxx, mxy) <= COORD_MAX) {
                e.ox0 = mnx - grow; e.oy0 = mny - grow; e.ox1 = mxx + grow; e.oy1 = mxy + grow;
                keep = e.ox0 <= tx1 && e.ox1 >= tx0 && e.oy0 <= ty1 && e.oy1 >= ty0;
                e.cx0 = e.cy0 = e.cx1 = e.cy1 = 0;
                e.lx = e.ly = e.lw = 0;
                e.loff = 0;
                if (lab_rect) {
                    const int lx = lab_rect[(size_t)r * 4], ly = lab_rect[(size_t)r * 4 + 1];
                    const int lw = lab_rect[(size_t)r * 4 + 2], lh = lab_rect[(size_t)r * 4 + 3];
                    if (lw > 0 && lh > 0) {
                        const long long x1 = min((long long)lx + lw, (long long)w), y1 = min((long long)ly + lh, (long long)h);
                        const int x0 = max(lx, 0), y0 = max(ly, 0);
                        if (x0 < x1 && y0 < y1) {        // some of it is inside the image
                            e.cx0 = x0; e.cy0 = y0; e.cx1 = (int)x1; e.cy1 = (int)y1;
                            e.lx = lx; e.ly = ly; e.lw = lw;
                            e.loff = lab_off[r];
                            keep = keep || (x0 <= tx1 && e.cx1 > tx0 && y0 <= ty1 && e.cy1 > ty0);
                        }
                    }
                }
                if (keep) e.color = (unsigned)color[(size_t)r * 4] | ((unsigned)color[(size_t)r * 4 + 1] << 8) |
                                    ((unsigned)color[(size_t)r * 4 + 2] << 16);
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int pos = __popcll(m & ((1ull << lane) - 1ull)), n = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = wave_cnt[k];
            if (k < wv) pos += c;
            n += c;
        }
        if (keep) list[pos] = e;                         // descending rows: a lower thread holds a higher row
        __syncthreads();

        for (int i = 0; i < n; i++) {
            if (__all(left == 0)) break;                 // this wave's pixels are all settled
            const Entry &s = list[i];
            const bool xo = gx <= s.ox1 && gx + 3 >= s.ox0, xl = gx < s.cx1 && gx + 4 > s.cx0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int y = gy + 16 * j;
                const bool yo = xo && y >= s.oy0 && y <= s.oy1, yl = xl && y >= s.cy0 && y < s.cy1;
                if (!(yo || yl)) continue;
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    if (res[4 * j + p] & DONE) continue;
                    const int x = gx + p;
                    bool cov = false;
                    if (yo && x >= s.ox0 && x <= s.ox1)
                        cov = edge_covers(x, y, s.q[0], s.q[1], s.q[2], s.q[3], t2) || edge_covers(x, y, s.q[2], s.q[3], s.q[4], s.q[5], t2) ||
                              edge_covers(x, y, s.q[4], s.q[5], s.q[6], s.q[7], t2) || edge_covers(x, y, s.q[6], s.q[7], s.q[0], s.q[1], t2);
                    if (!cov && yl && x >= s.cx0 && x < s.cx1)
                        cov = lab_bits[s.loff + (long long)(y - s.ly) * s.lw + (x - s.lx)] != 0;
                    if (cov) {
                        res[4 * j + p] = s.color | DONE;
                        left--;
                    }
                }
            }
        }
        if (__syncthreads_and(left == 0)) break;         // also the barrier before the next pass overwrites the list
    }

    const long long base = img_offset[b];
    const bool copy = dst != src;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = gy + 16 * j;
        if (y >= h || gx >= w) continue;
        const int nv = min(4, w - gx);
        bool painted = false;
#pragma unroll
        for (int p = 0; p < 4; p++) painted = painted || (p < nv && (res[4 * j + p] & DONE));
        if (!copy && !painted) continue;
        const long long a = base + ((long long)y * w + gx) * 3;
        const uint8_t *sp = src + a;
        uint8_t *dp = dst + a;
        unsigned px[4] = {0, 0, 0, 0};
        if (nv == 4 && !((uintptr_t)sp & 3)) {
            const unsigned w0 = ((const unsigned *)sp)[0], w1 = ((const unsigned *)sp)[1], w2 = ((const unsigned *)sp)[2];
            px[0] = w0 & 0xffffffu;
            px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
            px[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
            px[3] = w2 >> 8;
        } else {
#pragma unroll
            for (int p = 0; p < 4; p++)
                if (p < nv) px[p] = (unsigned)sp[3 * p] | ((unsigned)sp[3 * p + 1] << 8) | ((unsigned)sp[3 * p + 2] << 16);
        }
#pragma unroll
        for (int p = 0; p < 4; p++)
            if (p < nv && (res[4 * j + p] & DONE)) px[p] = res[4 * j + p] & 0xffffffu;
        if (nv == 4 && !((uintptr_t)dp & 3)) {
            ((unsigned *)dp)[0] = px[0] | (px[1] << 24);
            ((unsigned *)dp)[1] = (px[1] >> 8) | (px[2] << 16);
            ((unsigned *)dp)[2] = (px[2] >> 16) | (px[3] << 8);
        } else {
#pragma unroll
            for (int p = 0; p < 4; p++)
                if (p < nv) {
                    dp[3 * p] = (uint8_t)px[p];
                    dp[3 * p + 1] = (uint8_t)(px[p] >> 8);
                    dp[3 * p + 2] = (uint8_t)(px[p] >> 16);
                }
        }
    }
}

}  // namespace

extern "C" {

int ryolo_draw_rows_per_pass(void) { return ROWS_PER_PASS; }
int ryolo_draw_max_images(void) { return MAX_IMAGES; }

int ryolo_draw_quads(const uint8_t *src, uint8_t *dst, const long long *img_offset, const int *img_hw, int n_img, int max_h, int max_w,
                     const int *quad, const int *det_off, int M, const uint8_t *color, const int *thick, const uint8_t *lab_bits,
                     const long long *lab_off, const int *lab_rect, void *stream) {
    if (!src || !dst || !img_offset || !img_hw || !thick) return RYOLO_EINVAL;
    if (n_img < 1 || n_img > MAX_IMAGES || M < 0) return RYOLO_EINVAL;
    if (max_h < 1 || max_h > MAX_SIDE || max_w < 1 || max_w > MAX_SIDE) return RYOLO_EINVAL;
    if (M > 0 && (!quad || !det_off || !color)) return RYOLO_EINVAL;
    if ((uintptr_t)quad & 15) return RYOLO_EINVAL;
    const int labels = (lab_bits != nullptr) + (lab_off != nullptr) + (lab_rect != nullptr);
    if (labels != 0 && labels != 3) return RYOLO_EINVAL;
    Thick th;
    for (int b = 0; b < n_img; b++) {
        if (thick[b] < 1 || thick[b] > 255) return RYOLO_EINVAL;
        th.t[b] = (unsigned char)thick[b];
    }
    for (int b = n_img; b < MAX_IMAGES; b++) th.t[b] = 1;
    if (M == 0 && dst == src) return RYOLO_OK;
    const dim3 grid((max_w + TILE - 1) / TILE, (max_h + TILE - 1) / TILE, n_img);
    hipLaunchKernelGGL(draw_quads_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, dst, img_offset, img_hw, quad, det_off, M, color, th,
                       lab_bits, lab_off, lab_rect);
    return hipGetLastError() == hipSuccess ? RYOLO_OK : RYOLO_ELAUNCH;
}

}  // extern "C"
