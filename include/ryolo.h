/*
 * include/ryolo.h -- C ABI of libryolo_hip.so, the MI355X (gfx950) hot path of rotated-YOLOv3.
 *
 * Drop-in boundary.  The reference has exactly one FFI on this path, the pybind11 module `r_nms`
 * (utils/nms/src/rotate_polygon_nms.cpp:7-16, built by utils/nms/setup.py:4-13).  Everything else on the path
 * is reached through PyTorch operator calls (cuDNN conv / BN / PReLU in model/models.py:55-66, elementwise
 * decode in model/models.py:198-221).  Each entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - plain C: pointers are DEVICE pointers unless a parameter says "host"; sizes are element counts;
 *     `stream` is a hipStream_t passed as void* (NULL = the null stream).  No torch types.
 *   - every function only ENQUEUES work on `stream` and returns; nothing is allocated inside (the caller
 *     provides workspaces whose size the *_workspace_bytes functions report), so calls are hipGraph-capturable.
 *   - return value: 0 = RYOLO_OK, otherwise a negative RYOLO_E* code (ryolo_strerror gives the text).
 *     There is NO CPU fallback: without a gfx950 device the launch fails and the error is returned.
 */
#ifndef RYOLO_H
#define RYOLO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RYOLO_OK 0
#define RYOLO_EINVAL -1   /* bad argument (null pointer, negative size, unsupported shape) */
#define RYOLO_ELAUNCH -2  /* HIP reported an error while enqueuing */
#define RYOLO_ETOOBIG -3  /* n above RYOLO_RNMS_MAX_BOXES */

#define RYOLO_RNMS_MAX_BOXES 262144

const char *ryolo_strerror(int code);
/* ABI version; bumped when a signature or a contract changes.  3: ryolo_rnms_workspace_bytes grew (the split scan's state words) and
 * ryolo_set_tuning was added since 2; ryolo_rnms on a capturing stream runs unsplit.  4: ryolo_se_workspace_bytes / ryolo_se_nhwc added. */
int ryolo_abi_version(void);
/* "RYOLO_BUILD_ID=" + 16 hex digits: a hash of the library's sources, headers and compiler flags (__graft_entry__.source_id()). */
const char *ryolo_build_id(void);
/* The library's six tuning switches (dispatch selections for tests and A/B timing; none of them changes results beyond fp32 summation
 * order): RYOLO_CONV3X3 = mp | mq, RYOLO_CONV1X1 = igemm, RYOLO_RNMS_TILES = 1 | 2 (column tiles per wave of the NMS mask kernel),
 * RYOLO_MQ_KORDER = 0 | 1, RYOLO_BN_REDUCE_TILES = 0, RYOLO_STEM_DGRAD = 0..3.  Each is read from the environment once, at its first use; this call sets (value) or clears (NULL / "") one in
 * the running process.  Not synchronised with launches in flight on other threads.  RYOLO_EINVAL: unknown name. */
int ryolo_set_tuning(const char *name, const char *value);

/* ------------------------------------------------------------------------------------------------
 * Rotated NMS  -- replaces r_nms(dets, threshold) of utils/nms/src/rotate_polygon_nms.cpp:7-12
 *                 (-> nms_cuda, rotate_polygon_nms_kernel.cu:323-384; tile kernel :262-308; IoU :22-260).
 *
 *   dets        [n, >=6] float32 rows (cx, cy, w, h, angle_rad, score); `row_stride` = floats between rows
 *               (a column slice dc[:, :6] of an [n,8] tensor is passed as-is with row_stride 8, cf.
 *               utils/nms/nms.py:64; the reference compacts it with index_select, kernel.cu:328).
 *   thr         IoU threshold, suppression iff IoU > thr (strict, kernel.cu:301).
 *   keep_out    [n] int64, receives the kept ORIGINAL row indices in ascending order (kernel.cu:380-383).
 *   num_keep    [1] int32, receives K.
 *   workspace   ryolo_rnms_workspace_bytes(n) bytes of device scratch (contents irrelevant on entry).
 *
 * Semantics: sort by score descending (stable: ties keep the lower index first); box j is suppressed iff a
 * kept box i earlier in that order has devRotateIoU(box_i, box_j) > thr, box_i as first argument.
 * Bit-exact against oracle/riou_oracle.c (which is pinned to the reference arithmetic, tests/golden).
 * The reference's blocking D2H copy of the whole n x n/64 bit matrix and its host scan (kernel.cu:352-376)
 * are replaced by an on-device scan; only K (4 bytes) ever needs to reach the host.
 * Calls of more than 20 416 boxes run part of their work on a second, library-owned stream (the scan of the first block rows beside
 * the IoU kernel of the last ones); HIP events order it inside the call's position on `stream` -- for the caller the call is still
 * "enqueued on `stream`": everything enqueued on `stream` before it is visible to it, everything after it sees its results.
 * Stream rules of that split:
 *   - a call on a CAPTURING stream runs unsplit (asked with hipStreamIsCapturing on every call): a captured ryolo_rnms is a linear
 *     chain of launches on `stream` alone, whatever was called before it, and replays on whatever `dets` holds by then;
 *   - concurrent eager calls (several host threads, several streams) are serialised on one library stream per device -- the one
 *     mutex-guarded stream + two events of the calling thread's current device; each call needs its own workspace, keep_out and num_keep;
 *   - if an event call fails, the rest of the work is enqueued on `stream` in order and the call returns RYOLO_ELAUNCH.
 */
size_t ryolo_rnms_workspace_bytes(int n);
int ryolo_rnms(const float *dets, int n, int row_stride, float thr, int64_t *keep_out, int32_t *num_keep,
               void *workspace, size_t workspace_bytes, void *stream);

/* Segmented rotated NMS: `num_segments` independent sets stored back to back in `dets` (segment s = rows
 * [seg_offsets[s], seg_offsets[s+1]), device int32[num_segments+1]), each ALREADY sorted by score descending -- the
 * order in which the greedy scan visits a set (utils/nms/nms.py:57-66 sorts each image's class before calling r_nms).
 * One launch of each kernel covers all sets (a batch of images x classes).  keep_flags[i] = 1 iff row i survives in
 * its set.  max_seg_len >= the longest segment (host value; sizes the grid and the workspace).  Same arithmetic and
 * the same bit-exact bar as ryolo_rnms. */
size_t ryolo_rnms_segmented_workspace_bytes(int m, int num_segments, int max_seg_len);
int ryolo_rnms_segmented(const float *dets, int m, int row_stride, const int32_t *seg_offsets, int num_segments,
                         int max_seg_len, float thr, unsigned char *keep_flags, void *workspace, size_t workspace_bytes,
                         void *stream);

/* Weighted-merge rotated NMS -- the `nms_style == 'MERGE'` branch of the reference (utils/nms/nms.py:115-127): the kept box becomes the
 * score-weighted mean of the boxes it suppresses.  Input as ryolo_rnms_segmented; three outputs of m rows each (rows outside every
 * segment are left untouched in all three):
 *   keep_flags [m] uint8   bit-identical to what ryolo_rnms_segmented writes for the same input (the same kernels, tiles and scan).
 *   owner      [m] int32   kept row j: owner[j] = j.  Suppressed row j: the global row index of the smallest i < j of j's segment with
 *                          keep[i] and devRotateIoU(box_i, box_j) > thr -- the same fp32 value, box_i as first argument, and the same
 *                          strict comparison as the mask kernel's (above).  That is the reference's loop: a box belongs to the first kept
 *                          box at whose turn it is still alive and overlaps it.  The kept box is always a member of its own group (the
 *                          reference relies on IoU(b, b) > thr for that; this definition does not).
 *   merged     [m, 5] fp32 kept row i with members M(i) = { j : owner[j] = i } and weights w_j = score_j:
 *                          merged[i][f] = (sum_j w_j * v_j[f]) / (sum_j w_j) for f in cx, cy, w, h, a.  Products, sums and the one
 *                          division per field in fp64, the quotient rounded once to fp32.  The order of the sums is fixed by the members'
 *                          positions in their segment (no floating-point atomics): two calls on the same input give the same bits.  Rows that are not kept:
 *                          five zeros.  sum_j w_j not a finite number greater than 0: the kept row's own five fields.
 * Angles (the one deviation from the reference, which takes the plain mean): a box is unchanged by a -> a +- pi, so a member's angle
 * enters the sum as a_j - pi * rint((a_j - a_i) / pi), a_i the owner's angle, in fp64 with pi = 3.14159265358979323846 and rint to nearest
 * even: within pi/2 of a_i.  The merged angle is not wrapped back.  When every member is within pi/2 of its owner this is the reference's
 * arithmetic.  Score, class confidence and class are not this call's business; which rows survive is exactly what the plain call decides.
 * No polygon IoU is evaluated a second time: the owner comes from the tiles and summaries the mask kernel left in the workspace.  The call
 * is a linear chain of launches on `stream` (extent, corners, mask, scan, keep words, owner, merge, and two small memsets): no second
 * stream, no host synchronisation, no host read; capturable.  Arguments and return codes as ryolo_rnms_segmented; a NULL owner or merged is RYOLO_EINVAL. */
size_t ryolo_rnms_merge_segmented_workspace_bytes(int m, int num_segments, int max_seg_len);
int ryolo_rnms_merge_segmented(const float *dets, int m, int row_stride, const int32_t *seg_offsets, int num_segments,
                               int max_seg_len, float thr, unsigned char *keep_flags, int32_t *owner, float *merged /* [m,5] */,
                               void *workspace, size_t workspace_bytes, void *stream);

/* Measurement hook (bench.py's nms.roofline): while `device_counter` is non-NULL every subsequent ryolo_rnms /
 * ryolo_rnms_segmented call adds the number of box pairs whose exact polygon IoU it evaluated (pairs that survive the
 * bounding-circle reject) to *device_counter (uint64, zeroed by the caller).  NULL switches it off.  Not thread safe. */
void ryolo_rnms_count_pairs(uint64_t *device_counter);

/* ------------------------------------------------------------------------------------------------
 * Rotated IoU -- the arithmetic of devRotateIoU (kernel.cu:251-260) exposed directly; replaces the
 * per-pair Python/shapely loop of skew_bbox_iou (utils/utils.py:290-320) used by test.py:146.
 *   ryolo_riou_pairs : out[i]        = IoU(b1[i], b2[i])           i < n
 *   ryolo_riou_matrix: out[i*n2 + j] = IoU(b1[i], b2[j])           i < n1, j < n2
 * Rows are (cx, cy, w, h, angle_rad, ...) float32 with the given row strides (floats).
 */
int ryolo_riou_pairs(const float *b1, int stride1, const float *b2, int stride2, int n, float *out, void *stream);
int ryolo_riou_matrix(const float *b1, int n1, int stride1, const float *b2, int n2, int stride2, float *out,
                      void *stream);

/* Rotated IoU of the EVALUATION path -- replaces skew_bbox_iou (utils/utils.py:290-320: get_rotated_coors :702-725 + skewiou
 * :663-699, a per-pair Python loop over shapely polygon intersections in fp64) as called by test.py:146 for mAP matching.
 * Corners in fp64 with get_rotated_coors' rotation matrix, exact convex-polygon intersection (fp64 Sutherland-Hodgman clip),
 * inter / (area1 + area2 - inter), 0 when either area or the union is 0.  Differs from ryolo_riou_* (the NMS kernel's fp32
 * arithmetic, kept bit for bit) exactly where that arithmetic is not the geometric IoU: e.g. IoU(A, A) is 1 here.
 * Tolerance vs oracle/poly_iou.py: 1e-6 absolute. */
int ryolo_skew_iou_pairs(const float *b1, int stride1, const float *b2, int stride2, int n, float *out, void *stream);
int ryolo_skew_iou_matrix(const float *b1, int n1, int stride1, const float *b2, int n2, int stride2, float *out,
                          void *stream);

/* mAP matching of a whole batch -- replaces the per-image, per-prediction greedy loop of test.py:121-151 (one skew_bbox_iou call and a
 * `detected` list per prediction) by three launches for all images of a batch.
 *   det      [n_det, >=8] float32 rows (x, y, w, h, angle, score, class_conf, class) of all images, in image order and score-descending
 *            inside an image (what non_max_suppression returns, concatenated); `det_stride` = floats between rows.
 *   det_off  [n_img+1] int32: image k owns rows [det_off[k], det_off[k+1]); det_off[0] = 0, det_off[n_img] = n_det, non-decreasing.
 *   lab      [n_lab, >=6] float32 rows (class, x, y, w, h, angle) in pixels, in image order; lab_off [n_img+1] int32 likewise.
 *   correct  [n_det] uint8: 1 iff the reference's loop marks the prediction correct; matched [n_det] int32 (may be NULL): the row of
 *            `lab` a correct prediction detected, -1 otherwise.
 *   ws       ryolo_eval_match_workspace_bytes(n_det, n_lab) bytes of device scratch, 8-byte aligned (contents irrelevant on entry).
 * Semantics: for prediction i, best(i) = the label of its image with lab class == det class (float equality) and the largest IoU, the
 * lowest row on ties (torch.max(0)); the IoU is the fp32 value ryolo_skew_iou_matrix gives for the pair, bit for bit (the same fp64
 * operations in the same order); i claims best(i) iff that IoU > iou_thres, compared in fp32 (`tensor > python_float` rounds the
 * threshold to fp32); correct[i] = 1 iff i is the smallest claimant of best(i).  That IS the greedy loop: a label is marked detected only
 * by a correct prediction whose best it is, so its first claimant finds it free and every later one finds it taken.  A NaN IoU
 * (non-finite boxes only) makes its prediction claim nothing, as `NaN > thres` does.  No limit on predictions per image.
 * Launches (all on `stream`, deterministic -- the only atomics are integer minima): labels -> corners, predictions -> best + atomicMin,
 * predictions -> compare.  n_det == 0: nothing is launched; n_lab == 0: one launch writes correct = 0, matched = -1.
 * RYOLO_EINVAL, before anything is enqueued: a negative count, det_stride < 8, lab_stride < 6, iou_thres NaN / < 0 / >= 1, workspace_bytes
 * below the query, n_det > 0 with n_img == 0 or a null det / det_off / correct, n_det > 0 and n_lab > 0 with a null lab / lab_off or a null
 * or misaligned ws.  The workspace query returns 0 for a negative count. */
size_t ryolo_eval_match_workspace_bytes(int n_det, int n_lab);
int ryolo_eval_match(const float *det, int det_stride, const int32_t *det_off, const float *lab, int lab_stride, const int32_t *lab_off,
                     int n_img, int n_det, int n_lab, float iou_thres, uint8_t *correct, int32_t *matched /* may be NULL */, void *ws,
                     size_t ws_bytes, void *stream);


/* ------------------------------------------------------------------------------------------------
 * Convolution block -- replaces the operator chain the reference builds per `convolutional` cfg block,
 * nn.Conv2d -> nn.BatchNorm2d -> nn.PReLU (model/models.py:49-66), plus the `shortcut` add
 * (model/models.py:281-282) and the nearest `upsample` + `route` concat write (model/models.py:93-94,
 * :269-278) when they consume this block's output:
 *
 *     y = upsample( act( conv(x, W) * scale[c] + shift[c] ) + residual )
 *
 * Activations are NHWC bf16; a tensor may be a channel slice of a wider buffer (pixel stride `*_cstride`
 * elements >= its channel count), which is how route/concat outputs are written in place.
 * scale/shift: fp32 [ryolo_conv_cpad(Cout)] (eval-mode BatchNorm folded: scale = gamma/sqrt(var+eps),
 * shift = beta - mean*scale, cf. utils/torch_utils.py:45-69; or scale = 1, shift = bias for the head convs),
 * padded with zeros.  Arithmetic: bf16 x bf16 products accumulated in fp32 on MFMA; scale/shift/act in
 * fp32; rounded to bf16; the residual is added in fp32 and rounded to bf16 again (the value a layer-by-layer
 * bf16 execution of the reference produces).  Tolerance vs an fp32 reference on the same bf16 inputs: 2 bf16 ulp.
 * All pointers 16-byte aligned; Cin, Cout and the channel strides multiples of 8; ksize 1 (pad 0) or 3
 * (Cin a power of two or a multiple of 64); upsample 1 or 2.
 */
#define RYOLO_ACT_LINEAR 0
#define RYOLO_ACT_LEAKY 1 /* x > 0 ? x : slope * x  -- LeakyReLU(0.1) and the reference's PReLU(1) (models.py:63-66) */
#define RYOLO_ACT_MISH 2  /* x * tanh(softplus(x))  -- extension named by the north star, not in the reference */

typedef struct ryolo_conv_desc {
    int N, H, W;        /* input batch / height / width */
    int Cin, Cout;      /* channels as seen by the kernel (first layer: Cin padded 3 -> 8) */
    int ksize, stride, pad;
    int in_cstride, out_cstride, res_cstride; /* pixel strides in elements */
    int act;            /* RYOLO_ACT_* */
    float slope;
    int upsample;       /* 1, or 2: y has spatial size 2Ho x 2Wo, every result written to its 2x2 block */
    int tile;           /* low byte: 0 = auto; 1 = 128x128 (8 waves), 2 = 256x64, 3 = 256x32, 4 = 256x128 3-stage, 6 / 7 = 128x128 with
                         * 8 waves as 4x2 / 4 waves as 2x2 (pixels x channels per workgroup); 8 / 11 / 14 = the 256-channel
                         * multi-phase tile of conv_mp.hip with 256 / 192 / per-shape pixel rows, 9 = the 128 x 256 tile of
                         * conv_mq.hip; 12 = the stem kernel of conv_stem.hip (3x3, 32 -> 64 channels only), 13 = the weight-stationary 1x1 kernel of conv_pw.hip (two 4-wave workgroups per CU; same bits as 8 / 11); auto picks between them per launch
                         * (environment RYOLO_CONV3X3=mp|mq forces one family).  Test / tuning bits: 0x100 general address
                         * path, 0x200 never the persistent grid, 0x800 persistent grid also for 3x3;
                         * ryolo_conv2d_wgrad: 0x2000 the two-stage square tile instead of the three-stage tiles, 0x4000 the
                         * transposed 128 x 256 tile, bits 16+ : forced split count */
} ryolo_conv_desc;

/* bytes of the packed bf16 weight image [cpad(Cout)][kpad(ksize*ksize*Cin_pad)] (+ zero tail) */
size_t ryolo_conv_packed_weight_bytes(int Cout, int Cin_pad, int ksize);
/* w_oihw: fp32 [Cout][Cin][ksize][ksize] (the nn.Conv2d.weight layout, models.py:55) -> packed image */
int ryolo_conv_pack_weights(const float *w_oihw, int Cout, int Cin, int ksize, int Cin_pad, void *packed,
                            void *stream);
int ryolo_conv2d_bn_act(const ryolo_conv_desc *desc /* host */, const void *x, const void *w_packed,
                        const float *scale, const float *shift, const void *residual /* may be NULL */, void *y,
                        void *stream);
/* Two consecutive `convolutional` blocks (model/models.py:49-66, twice) in ONE launch when the tensor between them has no other
 * reader (inference): y = block_second(block_first(x)) [+ x when shortcut_from_input: the `shortcut` of models.py:281-282 whose
 * `from` is the first block's input].  The intermediate tensor is computed into LDS, rounded to bf16 as if it had been stored, and
 * never reaches HBM; the result is bit-identical to two ryolo_conv2d_bn_act calls.  Served pair (ryolo_conv_pair_supported):
 * Darknet-53 layers 2-4 (1x1 64->32, then 3x3 32->64 + shortcut).
 * Descriptors as for ryolo_conv2d_bn_act; second->out_cstride is y's pixel stride; no residual operand besides the shortcut. */
int ryolo_conv_pair_supported(const ryolo_conv_desc *first, const ryolo_conv_desc *second, int shortcut_from_input);
int ryolo_conv2d_bn_act_pair(const ryolo_conv_desc *first, const ryolo_conv_desc *second, const void *x, const void *w_first,
                             const float *scale_first, const float *shift_first, const void *w_second, const float *scale_second,
                             const float *shift_second, int shortcut_from_input, void *y, void *stream);
/* Which kernel ryolo_conv2d_bn_act (with_statistics: ryolo_conv2d_bn_act_stats) would launch for this descriptor on the current
 * device -- the plan the launch would execute, nothing is enqueued.  For benchmarks and profiles (the per-kernel tables name the kernel
 * that actually ran); -1 for an invalid descriptor. */
#define RYOLO_CONV_KERNEL_MP256 1   /* conv_mp.hip, 256 pixels x 256 channels, one 8-wave workgroup per CU */
#define RYOLO_CONV_KERNEL_MP192 2   /* conv_mp.hip, 192 x 256 */
#define RYOLO_CONV_KERNEL_MQ 3      /* conv_mq.hip, 128 x 256, two 4-wave workgroups per CU */
#define RYOLO_CONV_KERNEL_DIRECT8 4 /* first layer (C_in 3 -> 8), fragments straight from global memory */
#define RYOLO_CONV_KERNEL_STEM 5    /* conv_stem.hip: 3x3, 32 -> 64 channels, stride 1 / 2: input patch staged once, filter in registers */
#define RYOLO_CONV_KERNEL_PW 6      /* conv_pw.hip: 1x1 stride 1, the filter slice in registers, rows through an LDS ring */
#define RYOLO_CONV_KERNEL_STEM0 8   /* conv_stem.hip: the first layer's forward with its input patch staged in LDS (statistics passes keep DIRECT8) */
#define RYOLO_CONV_KERNEL_STEM_DGRAD 7 /* conv_stem.hip: the data gradient of a 3x3 32 -> 64 stem layer (stride 2: all four parity classes) in one launch */
#define RYOLO_CONV_KERNEL_STEM64 11 /* conv_stem.hip: 3x3 / 1, 64 -> 128: input patch staged once, the filter split over the waves' registers */
#define RYOLO_CONV_KERNEL_MQ128 9   /* conv_mq.hip, 128 pixels x 128 channels (round 5): layers / data gradients with C_out % 256 != 0 */
#define RYOLO_CONV_KERNEL_MQ64 10   /* conv_mq.hip, 64 pixels x 128 channels: short tile lists (1x1 layers at 19^2 / 38^2) */
#define RYOLO_CONV_KERNEL_IGEMM 16  /* + tile code of conv.hip's 128x128 / 256x64 / 256x32 ... tiles */
int ryolo_conv_kernel_choice(const ryolo_conv_desc *desc, int with_residual, int with_statistics);
/* The same query for the data gradient of `forward_desc` (ryolo_conv2d_dgrad; stride 2: the choice of the last parity class)
 * and for its weight gradient (ryolo_conv2d_wgrad): 32 / 64 / 128 = the square two-stage tile, 256 / 257 / 258 / 259 / 260 = the
 * three-stage tile 256x128 / 128x256 / 128x(3 taps x 64) / 128x128 / 64x128 (c_out x c_in), RYOLO_WGRAD_KERNEL_TAPS + v = the stem's per-tap kernels.
 * bench.py names the kernels of its in-run train-step table through them. */
#define RYOLO_WGRAD_KERNEL_TAPS 1000
int ryolo_conv_dgrad_kernel_choice(const ryolo_conv_desc *forward_desc, int with_bn_reduce /* ryolo_conv2d_dgrad_bnreduce's choice */);
int ryolo_conv_wgrad_kernel_choice(const ryolo_conv_desc *forward_desc);
/* Dilated 3x3 convolution (inference, csrc/conv_dil.hip) -- replaces F.conv2d(x, module_list[s].Conv2d.weight, padding=(dil_h, dil_w),
 * dilation=(dil_h, dil_w)), what the reference computes for a `d-convolutional` block with `weight_from = s` (model/models.py:254-267,
 * the "matrix" cfgs): tap (r, s) of output pixel (ho, wo) reads input pixel (ho + (r-1)*dil_h, wo + (s-1)*dil_w), zero outside the
 * image; the output is H x W.  Epilogue, arithmetic, layouts and the stream contract as for ryolo_conv2d_bn_act:
 * y = bf16(act(acc * scale[c] + shift[c])), then bf16(y + residual) when a residual is given.  w_packed is the image
 * ryolo_conv_pack_weights makes for the (undilated) 3x3 layer: one packed copy serves the source layer and all its sharers.
 * Served (ryolo_conv2d_dilated_supported, no device call): ksize 3, stride 1, pad 1 (the field names the undilated window; the
 * padding applied is the dilation), upsample 1, Cin % 64 == 0, Cout % 8 == 0, 1 <= dil_h, dil_w <= 32, act linear or leaky, channel
 * strides multiples of 8 and at least the channel counts (res_cstride too when a residual is given), all pointers 16-byte aligned,
 * tensors below 2 GiB.  Anything else: RYOLO_EINVAL before any HIP call.  `tile` is ignored.  One writer per output element and a
 * fixed summation order: results are bit-identical from run to run and do not depend on the batch size. */
int ryolo_conv2d_dilated_supported(const ryolo_conv_desc *desc, int dil_h, int dil_w);
int ryolo_conv2d_dilated(const ryolo_conv_desc *desc, int dil_h, int dil_w, const void *x, const void *w_packed, const float *scale,
                         const float *shift, const void *residual /* may be NULL */, void *y, void *stream);
/* Data gradient of that dilated convolution (training, csrc/conv_dil.hip) -- replaces what autograd computes for the F.conv2d of a
 * `d-convolutional` block with `weight_from` (model/models.py:254-267) with respect to its input:
 *     dx[n,h,w,ci] = sum_{r,s,co} dz[n, h-(r-1)*dil_h, w-(s-1)*dil_w, co] * W[co,ci,r,s],
 * the same dilated convolution applied to dz with the spatially flipped, channel-transposed filter, on the same kernel.  forward_desc
 * describes the FORWARD conv (dx has its input's geometry and pixel stride in_cstride); the calling convention is ryolo_conv2d_dgrad's
 * without `accumulate`: dz NHWC bf16 with pixel stride dz_cstride, ones / zeros fp32 [ryolo_conv_cpad(Cin)].  packed_dgrad is the
 * stride-1 image of ryolo_conv_pack_weights_dgrad for the source layer's weight, which for the served shapes is bit-equal to
 * ryolo_conv_pack_weights applied to W.flip(2,3).transpose(0,1): one packed copy serves the source layer's own data gradient and every
 * sharer's.  Served (ryolo_conv2d_dilated_dgrad_supported, no device call; dz's stride taken as out_cstride): the forward is served and
 * Cout % 64 == 0 (it is the K channel count here), Cin % 8 == 0.  Anything else: RYOLO_EINVAL before any HIP call.  dx is written once:
 * one writer per element and a fixed summation order, bit-identical from run to run and independent of the batch size. */
int ryolo_conv2d_dilated_dgrad_supported(const ryolo_conv_desc *forward_desc, int dil_h, int dil_w);
int ryolo_conv2d_dilated_dgrad(const ryolo_conv_desc *forward_desc, int dil_h, int dil_w, const void *dz, int dz_cstride,
                               const void *packed_dgrad, const float *ones, const float *zeros /* fp32 [cpad(Cin)] */, void *dx,
                               void *stream);
/* Weight gradient of the dilated convolution (training, csrc/wgrad_dil.hip) -- autograd's gradient of the same F.conv2d with respect to
 * the shared weight:
 *     dW[co,ci,r,s] (+)= sum_{n,h,w} dz[n,h,w,co] * x[n, h+(r-1)*dil_h, w+(s-1)*dil_w, ci],   zero outside the image.
 * x (pixel stride forward_desc->in_cstride) and dz (pixel stride dz_cstride) are NHWC bf16, possibly channel slices; grad_oihw is the fp32
 * [Cout][Cin][3][3] gradient.  MFMA over the pixels, split over pixel chunks into fp32 partial tiles in `workspace`
 * (ryolo_conv2d_dilated_wgrad_workspace_bytes; any contents on entry), reduced by one launch in a fixed order: no atomics, results are
 * bit-identical from run to run; the split count depends on the shape alone.  accumulate = 0 overwrites grad_oihw, accumulate = 1 adds:
 * the sharers of one source weight accumulate into it in launch order.  Served (ryolo_conv2d_dilated_wgrad_supported, no device call;
 * dz's stride taken as out_cstride): ksize 3, stride 1, pad 1, upsample 1, Cin % 64 == 0, Cout % 8 == 0 (a ragged last C_out tile: the
 * rows past Cout are not stored), 1 <= dil_h, dil_w <= 32, channel strides multiples of 8 and at least the channel counts, x / dz /
 * workspace 16-byte aligned, tensors below 2 GiB.  Anything else (a short workspace, a null pointer): RYOLO_EINVAL before any HIP call;
 * the workspace query returns 0.  `tile`, `act` are ignored.  Only enqueues on `stream`, allocates nothing. */
int ryolo_conv2d_dilated_wgrad_supported(const ryolo_conv_desc *forward_desc, int dil_h, int dil_w);
size_t ryolo_conv2d_dilated_wgrad_workspace_bytes(const ryolo_conv_desc *forward_desc, int dil_h, int dil_w);
int ryolo_conv2d_dilated_wgrad(const ryolo_conv_desc *forward_desc, int dil_h, int dil_w, const void *x, const void *dz, int dz_cstride,
                               float *grad_oihw, int accumulate, void *workspace, size_t workspace_bytes, void *stream);
/* layout converters at the model boundary: the reference feeds NCHW fp32 images (train.py:236, detect.py:209) */
int ryolo_nchw_f32_to_nhwc_bf16(const float *x, int N, int C, int H, int W, int Cpad, void *y, void *stream);
int ryolo_nhwc_bf16_to_nchw_f32(const void *x, int N, int C, int H, int W, int cstride, float *y, void *stream);

/* Real-data input (csrc/augment.hip) -- replaces, on the device, what LoadImagesAndLabels.__getitem__ does to the pixels of one image
 * (utils/datasets.py:431-451 letterbox, :470-484 + utils/augment.py the Transform chain, :498-500 the [0, 1] scaling): one launch turns
 * N cached uint8 images into the engines' input, bf16 [N][H][W][8] with channels 3..7 zero -- bit for bit what
 * ryolo_nchw_f32_to_nhwc_bf16 makes of the fp32 image when the map is the identity.
 *   pixels      the cache: RGB uint8 HWC images of different sizes, back to back; image i starts at byte img_offset[i] and is
 *               img_hw[i] = (h, w) pixels.  src_index[n] selects the cached image of batch slot n (one outside [0, n_cache) reads
 *               nothing: the slot is all border).
 *   params      [N][ryolo_aug_nparam() = 16] fp32 rows: m00 m01 m02 m10 m11 m12 | noise_sigma | gamma | gamma_max | blur_sigma |
 *               sat_gain | val_gain | gray_alpha | three reserved zeros.  The matrix maps an OUTPUT pixel index (x, y) to source pixel
 *               coordinates, sx = m00 x + m01 y + m02, sy = m10 x + m11 y + m12: letterbox resize and padding, the random affine and both
 *               flips are folded into it by the host.  Neutral: 0, 1, any, 0, 1, 1, 0; a neutral stage is skipped, exactly.
 *   seed        keys the noise: a counter-based hash of (seed, n, y, x), no state, the same call gives the same bits.
 * Stages, fp32 on a 0..255 scale, never quantised in between (the full definition, with the hash written out in 32-bit operations, is
 * the header comment of csrc/augment.hip; tests/augment_reference.py restates it in float64):
 *   bilinear sample, taps outside the source = 128  ->  + noise_sigma * z (one z per pixel), clamp  ->  powf(v / gamma_max, gamma) *
 *   gamma_max  ->  separable Gaussian blur over the output grid, taps |d| <= 4, BORDER_REFLECT_101, blur_sigma above
 *   ryolo_aug_max_blur_sigma() = 1.5 taken as that  ->  saturation / value gains in the hue-free closed form  ->  blend towards
 *   0.299 R + 0.587 G + 0.114 B by gray_alpha  ->  clamp, / 255.0f, round to nearest even bf16.
 * One launch on `stream`: 256-thread workgroups own 32 x 32 output tiles; no workspace, no allocation, no atomics, one writer per
 * element, capture-safe, bit-identical from run to run.  RYOLO_EINVAL before any HIP call: a null pointer (other than stream), N, H, W
 * or n_cache < 1, N or the row-tile count above 65535, y not 16-byte aligned.  The two queries need no device. */
int ryolo_aug_nparam(void);
float ryolo_aug_max_blur_sigma(void);
int ryolo_letterbox_augment(const uint8_t *pixels, const long long *img_offset, const int *img_hw /* [n_cache][2] */, int n_cache,
                            const int *src_index /* [N] */, const float *params /* [N][16] */, long long seed, int N, int H, int W,
                            void *y /* bf16 [N][H][W][8] */, void *stream);

/* Detection input (csrc/letterbox_area.hip) -- letterbox(img0, new_shape) of the reference's detect.py (utils/datasets.py:431-451) on the
 * device, from the ORIGINAL pixels to any size: the cache layout, src_index and the output (bf16 [N][H][W][8], channels 3..7 zero, one
 * 16-byte store per pixel) are those of ryolo_letterbox_augment; a src_index outside [0, n_cache) makes the slot all border.
 *   place       HOST memory, [N][4] rows (left, top, new_w, new_h): slot n shows its image resized to new_w x new_h with the top left
 *               corner at output pixel (left, top).  Read and validated during the call and passed on in the kernel arguments (64 slots per
 *               launch), so a captured graph replays the rows it was captured with.
 * Output pixel (x, y) with left <= x < left + new_w and top <= y < top + new_h is inside the picture; every other one is 128 exactly (a
 * hard edge, as cv2.copyMakeBorder makes).  Inside, the value is the separable sum  (sum_j Wy_j ((sum_i Wx_i p[j][i]) / Dx)) / Dy  per
 * channel, with integer weights per axis (source length s, output length n, output index k):
 *   n <  s   exact coverage: taps i from (k s) div n while i n < (k + 1) s, W = min((k + 1) s, (i + 1) n) - max(k s, i n), D = s (64-bit);
 *   n >= s   bilinear with aligned pixel centres: c = (2 k + 1) s - n, q = floor(c / 2n), r = c - 2n q; taps q, q + 1 clamped to
 *            [0, s - 1], W = (2n - r, r), D = 2n; n == s is the pixel itself.
 * fp32 on a 0..255 scale, sums from the first tap up, no uint8 rounding; then c / 255.0f (a division) and round to nearest even bf16.  The
 * full definition is the header comment of csrc/letterbox_area.hip; tests/letterbox_area_reference.py restates it in float64.
 * ceil(N / 64) launches on `stream`: 256-thread workgroups own 32 x 32 output tiles; no workspace, no allocation, no atomics, one writer
 * per element, capture-safe, bit-identical from run to run.  RYOLO_EINVAL before any HIP call: a null pointer (other than stream), N, H, W
 * or n_cache < 1, N or the row-tile count above 65535, y not 16-byte aligned, a place row with new_w or new_h < 1 or whose rectangle is
 * not inside H x W. */
int ryolo_letterbox_area(const uint8_t *pixels, const long long *img_offset, const int *img_hw /* [n_cache][2] */, int n_cache,
                         const int *src_index /* [N] */, const int *place /* host [N][4]: left, top, new_w, new_h */, int N, int H, int W,
                         void *y /* bf16 [N][H][W][8] */, void *stream);

/* Detection output (csrc/detpost.hip) -- what the reference's detect.py does to every detection in Python, one launch per batch each.
 * Both make no launch and return RYOLO_OK when M == 0; both are capture-safe, without workspace or atomics.
 * ryolo_det_rescale: scale_coords(...).round() (utils/utils.py:181-189) in place on flat rows [M][8]: row r belongs to image b with
 *   det_off[b] <= r < det_off[b + 1]; geom[b] = (gain, pad_x, pad_y) -- gain = S / max(h0, w0), pad_x = (S - w0 gain) / 2, pad_y alike,
 *   computed by the host in double and stored as fp32.  Columns 0, 1 become rintf((v - pad) / gain), columns 2, 3 rintf(v / gain), a
 *   true fp32 division; columns 4..7 are untouched.
 * ryolo_det_quads: xywha2icdar (utils/ICDAR/icdar_utils.py:105-135) per row in fp64 -- the four corners turned by cos(-a), sin(-a),
 *   order_points (stable sort by x; the two left-most by y are tl, bl; of the two right-most the one farther from tl is br, on a tie the
 *   later one), then tl, tr, br, bl truncated toward zero to int32.
 * RYOLO_EINVAL: M < 0, bs < 1, and for M > 0 a null pointer (other than stream) or det / quad not 16-byte aligned. */
int ryolo_det_rescale(float *det /* [M][8], in place */, int M, const int *det_off /* [bs+1], device */, int bs,
                      const float *geom /* [bs][3]: gain, pad_x, pad_y, device */, void *stream);
int ryolo_det_quads(const float *det /* [M][8] */, int M, int *quad /* [M][8] */, void *stream);
/* ryolo_det_corners: get_rotated_coors (utils/utils.py:702-725) per row in fp64 -- the arithmetic of ryolo_det_quads up to, but not
 *   including, order_points: the corners (xmin, ymin), (xmin, ymax), (xmax, ymax), (xmax, ymin) turned by cos(-a), sin(-a), kept in THAT
 *   order (a cycle; corner 0 anchors the drawn label) and truncated toward zero to int32, as .astype(np.int32) truncates.  The outline
 *   ryolo_draw_quads draws.  Arguments, M == 0 and capture safety as for ryolo_det_quads. */
int ryolo_det_corners(const float *det /* [M][8] */, int M, int *quad /* [M][8] */, void *stream);

/* Drawing (csrc/draw.hip) -- plot_one_box / plot_images of the reference (utils/utils.py:479-490, :514-550) on the device: rotated
 * outlines and label bitmaps painted into the pixels of an image cache (uint8 RGB HWC, image b at img_offset[b] bytes, img_hw[b] = (h, w)).
 * Row r of quad / color / lab_* belongs to image b with det_off[b] <= r < det_off[b + 1].  The three bytes of pixel P = (x, y) of image b in
 * dst are color[r*], r* the LARGEST row of the image that covers P (later rows paint over earlier ones); with no such row, those of src.
 *   outline  Q0..Q3 = quad[r] (ryolo_det_corners), t = thick[b].  r covers P when for an edge A = Qk, B = Q(k+1 mod 4) the squared distance
 *            from P to the closed segment AB has 4 dist^2 <= t^2, in exact integers: d = B - A, L2 = d.d, u = (P - A).d;  u <= 0 or L2 = 0:
 *            4 |P - A|^2 <= t^2;  u >= L2: 4 |P - B|^2 <= t^2;  else c = (P - A) x d and 4 c^2 <= t^2 L2.  A thick polyline with round
 *            joints and caps of diameter t; t = 1 leaves no gap in any line.  This definition is the port's own: cv2.polylines is not
 *            matched pixel for pixel.  A row with a corner coordinate outside [-16384, 32767] draws nothing, its label neither.
 *   label    lab_rect[r] = (lx, ly, lw, lh): r covers P when lx <= x < lx + lw, ly <= y < ly + lh and
 *            lab_bits[lab_off[r] + (y - ly) lw + (x - lx)] != 0 -- one byte per label pixel; the rectangle may lie partly or wholly outside
 *            the image; lw = 0 or lh = 0: no label for the row.  All three label pointers NULL: no labels at all.
 *   thick    HOST memory, [n_img], each 1..255: read and validated during the call and passed on in the kernel arguments, so a captured
 *            graph replays the thicknesses it was captured with (like `place` of ryolo_letterbox_area).
 *   max_h, max_w   at least the largest img_hw (host values: they size the grid, nothing on the device is read by the host); 1..16384.
 * dst == src is allowed (in place), otherwise the two must not overlap.  One launch: a 256-thread workgroup owns a 64 x 64 tile of one
 * image, culls the image's rows against it in passes of ryolo_draw_rows_per_pass() = 256 rows into an LDS list and every pixel stops at
 * the first (highest) row that covers it.  No workspace, no allocation, no atomics, one writer per byte, bytes of dst outside the images
 * are not touched, capture-safe, bit-identical from run to run.  M == 0: with dst == src no launch, otherwise a copy of the images.
 * RYOLO_EINVAL before any HIP call: a null src, dst, img_offset, img_hw or thick; n_img < 1 or above ryolo_draw_max_images() = 1024;
 * M < 0; M > 0 with a null quad, det_off or color; quad not 16-byte aligned; a thick entry outside 1..255; max_h or max_w outside
 * 1..16384; only some of the three label pointers.  The two queries need no device.  tests/draw_reference.py restates the definition. */
int ryolo_draw_rows_per_pass(void);
int ryolo_draw_max_images(void);
int ryolo_draw_quads(const uint8_t *src, uint8_t *dst, const long long *img_offset, const int *img_hw /* [n_img][2] */, int n_img,
                     int max_h, int max_w, const int *quad /* [M][8] */, const int *det_off /* [n_img+1] */, int M,
                     const uint8_t *color /* [M][4] RGBx */, const int *thick /* host [n_img] */, const uint8_t *lab_bits,
                     const long long *lab_off /* [M] */, const int *lab_rect /* [M][4]: x, y, w, h */, void *stream);


/* Decode + score filter + compaction (no `io` tensor): the rows of ryolo_yolo_decode's `io` that the first half of
 * non_max_suppression keeps (utils/nms/nms.py:33-48: class_conf/class = max over io[6:], score = io[5]*class_conf,
 * score > conf_thres, w,h > min_wh, all finite).  Survivors are appended to cand[capacity][8] =
 * (x, y, w, h, angle, score, class_conf, class) in arbitrary order, cand_row[slot] = image * io_rows_per_image +
 * io_row_offset + row (sort on it to get the reference's order); *counter (zeroed by the caller, shared by the heads of one
 * forward) counts survivors and may exceed `capacity` (then the tail was dropped: re-run with more room). */
int ryolo_yolo_decode_filter(const void *head, int head_cstride, int bs, int ny, int nx, int na, int no,
                             const float *anchors, float stride, float context_factor, int arc, float conf_thres,
                             float min_wh, long long io_rows_per_image, long long io_row_offset, float *cand,
                             long long *cand_row, int *counter, int capacity, void *stream);

/* ------------------------------------------------------------------------------------------------
 * YOLO head decode -- replaces YOLOLayer.forward (model/models.py:183-227) and create_grids
 * (model/model_utils.py:16-35).  `head`: NHWC bf16 output of the last 1x1 conv, channel = a*no + k, no = nc+6.
 *   io [bs, io_rows_per_image, no] fp32: rows io_row_offset + (a*ny + y)*nx + x receive the decoded
 *        (x, y, w, h, angle, obj, cls...) in pixels (the three heads write into one tensor: the torch.cat of
 *        models.py:298 becomes a row offset); may be NULL when p is given and the head meets the tiled kernel's
 *        conditions -- na*no and the head stride multiples of 8, `head` 16-byte aligned, 32 pixels of na*no bf16 channels within
 *        64 KiB (na*no <= 1024), no <= 96 -- otherwise RYOLO_EINVAL (the training forward only needs p);
 *   p  [bs, na, ny, nx, no] fp32 (may be NULL): the raw head values, the "training output" of models.py:189-194.
 *   anchors [na][3] fp32 = (w_px, h_px, angle_rad) (utils/parse_config.py:6-31 rows selected by the yolo mask);
 *   stride = img_size / grid (model_utils.py:20); context_factor = hyp['context_factor'] (models.py:207-208);
 *   arc: 0 'default*' (sigmoid obj+cls), 1 '*BCE*' (sigmoid cls, obj = 1), 2 '*CE*' (models.py:210-218).  The reference's CE line
 *        assigns nc+2 softmax values to nc+1 columns and raises; the definition is the torch backend's (rotate-yolov3_amd/model/models.py,
 *        YOLOLayer.forward): cls = softmax over [obj, cls...] without its first entry, obj = 1.  nc == 1 sets the class column to 1 last.
 */
int ryolo_yolo_decode(const void *head, int head_cstride, int bs, int ny, int nx, int na, int no,
                      const float *anchors, float stride, float context_factor, int arc, float *io,
                      long long io_rows_per_image, long long io_row_offset, float *p, void *stream);

/* A YOLO head in one launch (inference): the last 1x1 conv of a head (model/models.py:49-66 without BatchNorm: scale = 1, shift =
 * bias, linear) and YOLOLayer.forward (models.py:183-227) on its values.  The conv's results are rounded to bf16 -- the head tensor
 * ryolo_conv2d_bn_act would have stored -- into an on-chip tile and decoded there with the arithmetic of ryolo_yolo_decode; io / p
 * are bit-identical to conv + decode, and the head tensor (186 MB for the 76^2 head at bs 32) is never written or re-read.
 * Served (ryolo_conv_head_decode_supported, which runs the launch's own configuration test on the current device): C_in 256, 512 or 1024
 * (the three heads of yolov3.cfg), na*no <= 512, no 7 or 8.  Arguments as for the two calls it replaces. */
int ryolo_conv_head_decode_supported(const ryolo_conv_desc *desc, int na, int no);
int ryolo_conv_head_decode(const ryolo_conv_desc *desc, const void *x, const void *w_packed, const float *scale, const float *shift,
                           const float *anchors, int na, int no, float stride, float context_factor, int arc, float *io,
                           long long io_rows_per_image, long long io_row_offset, float *p, void *stream);
/* The training form of the same launch (served for the shapes ryolo_conv_head_decode_supported accepts): the training forward needs
 * the raw head values p [bs, na, ny, nx, no] fp32 (the p-only form of ryolo_yolo_decode) AND the bf16 head tensor itself, which the
 * loss and the backward read.  The on-chip head tile is written out twice -- as p rows and as NHWC rows of `head` (pixel stride
 * head_cstride, a multiple of 8; channels >= C_out are not touched) -- instead of being stored by the conv and re-read by the decode.
 * head and p are bit-identical to ryolo_conv2d_bn_act + ryolo_yolo_decode. */
int ryolo_conv_head_decode_store(const ryolo_conv_desc *desc, const void *x, const void *w_packed, const float *scale, const float *shift,
                                 int na, int no, void *head, int head_cstride, float *p, void *stream);

/* NHWC bf16 helpers for cfg graphs whose shortcut / upsample / route / maxpool cannot be fused into a conv
 * epilogue (model/models.py:79-94, :269-282).  Channel counts and strides multiples of 8.
 * ryolo_add_nhwc: y = bf16(float(a) + float(b)); y may alias a or b exactly (same pointer, same stride: each element is read by the
 * one thread that then writes it), which the training engine uses to accumulate in place; partially overlapping tensors are not allowed. */
int ryolo_add_nhwc(const void *a, int a_cstride, const void *b, int b_cstride, void *y, int y_cstride,
                   long long npix, int C, void *stream);
int ryolo_upsample_nhwc(const void *x, int x_cstride, void *y, int y_cstride, int N, int H, int W, int C, int scale,
                        void *stream); /* scale 1 = slice copy */
int ryolo_maxpool_nhwc(const void *x, int x_cstride, void *y, int y_cstride, int N, int H, int W, int C, int ksize,
                       int stride, void *stream);

/* Squeeze-and-excitation block (inference) -- replaces SELayer.forward (model/models.py:27-31):
 *   m[n,c] = mean over H,W of x[n,c,:,:];  g[n,:] = sigmoid(W2 . relu(W1 . m[n,:]));  y[n,c,h,w] = x[n,c,h,w] * g[n,c].
 *   x, y        NHWC bf16 [N, H, W, C]; either may be a channel slice of a wider buffer: `*_cstride` = elements between pixels,
 *               >= C and a multiple of 8, base address 16-byte aligned.  y must not overlap x (the block's input has a second reader,
 *               the residual skip): two disjoint channel slices of one buffer are fine.
 *   w1          fp32 [hidden][C]  = fc.0.weight (nn.Linear(C, C/16, bias=False), models.py:21);
 *   w2          fp32 [C][hidden]  = fc.2.weight (nn.Linear(C/16, C, bias=False), models.py:23).
 *   gate_out    fp32 [N][C] (may be NULL): receives g.
 *   workspace   ryolo_se_workspace_bytes(N, H, W, C) bytes of device scratch, 16-byte aligned (contents irrelevant on entry).
 * Arithmetic: the mean, both products and the sigmoid 1 / (1 + expf(-t)) are fp32 on the bf16 values of x; y is rounded to bf16 once.
 * The pixel sum is split into chunks that depend on (H, W, C) alone and is combined in a fixed order without atomics: results are
 * bit-identical from run to run and do not depend on the batch size.  Three launches on `stream` (pool partial sums, gate, scale).
 * Served: C % 8 == 0, 16 <= C <= 2048, 1 <= hidden <= 128, N <= 65535.  RYOLO_EINVAL: a null pointer (other than gate_out), a size
 * outside these, a misaligned pointer or stride, workspace_bytes below the reported size, y overlapping x.  The workspace query
 * returns 0 for a shape that is not served. */
size_t ryolo_se_workspace_bytes(int N, int H, int W, int C);
int ryolo_se_nhwc(const void *x, int x_cstride, const float *w1 /* fp32 [hidden][C] */, const float *w2 /* fp32 [C][hidden] */,
                  int hidden, void *y, int y_cstride, int N, int H, int W, int C,
                  float *gate_out /* fp32 [N][C], may be NULL */, void *workspace, size_t workspace_bytes, void *stream);
/* Backward of that block (training, csrc/se_bwd.hip) -- replaces what autograd computes for SELayer.forward.  Saved from the forward: x
 * and the two weights; the gate is recomputed, by the forward's code in the forward's order (gate_out here is bit-equal to ryolo_se_nhwc's
 * on the same x).  Given dy (NHWC bf16), with m, u = W1 . m, z = relu(u), g as above; every sum and product fp32 on the bf16 values:
 *     s[n,c]  = sum_hw dy * x                       dt = s * g * (1 - g)
 *     dW2[c,h] (+)= sum_n dt[n,c] * z[n,h]          dz[n,h] = sum_c dt[n,c] * W2[c,h]     du = dz where z > 0, else 0
 *     dW1[h,c] (+)= sum_n du[n,h] * m[n,c]          dm[n,c] = sum_h du[n,h] * W1[h,c]
 *     dx = bf16(float(dy) * g + dm / (H*W))         one rounding; dx_accumulate = 1 adds float(dx's old value) before that rounding
 *   x, dy, dx   NHWC bf16 [N, H, W, C], each possibly a channel slice (`*_cstride` >= C, a multiple of 8, base 16-byte aligned).  dx may be
 *               NULL: no data gradient.  dx must overlap neither x nor dy, by ryolo_se_nhwc's rule (two disjoint channel slices of one
 *               buffer do not overlap).
 *   dw1, dw2    fp32 [hidden][C] / [C][hidden]; both NULL: no weight gradients (one alone NULL: RYOLO_EINVAL).  accumulate_w = 0 overwrites
 *               them (any contents on entry), 1 adds the batch's sum to the old value with one fp32 add per element.
 *   gate_out    fp32 [N][C] (may be NULL): receives g.
 *   workspace   ryolo_se_bwd_workspace_bytes(N, H, W, C, hidden) bytes of device scratch, 16-byte aligned (contents irrelevant on entry).
 * At most four launches on `stream` (pixel sums of x and dy * x per chunk; gate and the per-image vectors; weight gradients, when wanted;
 * dx, when wanted); nothing is allocated.  The chunking depends on (H, W, C) alone, the sums over chunks, channels, hidden units and
 * images run in a fixed order and there are no atomics: every output is bit-identical from run to run, and dx / gate_out of an image do
 * not depend on the batch it is in.  Served: ryolo_se_nhwc's range (C % 8 == 0, 16 <= C <= 2048, 1 <= hidden <= 128, N <= 65535).
 * RYOLO_EINVAL, before anything is enqueued: a null x / dy / w1 / w2 / workspace, dx and both dw* all NULL, a size outside the range, a
 * misaligned pointer or stride, workspace_bytes below the reported size, dx overlapping x or dy.  The workspace query returns 0 for a shape
 * that is not served. */
size_t ryolo_se_bwd_workspace_bytes(int N, int H, int W, int C, int hidden);
int ryolo_se_bwd_nhwc(const void *x, int x_cstride, const void *dy, int dy_cstride, const float *w1 /* fp32 [hidden][C] */,
                      const float *w2 /* fp32 [C][hidden] */, int hidden, void *dx /* may be NULL */, int dx_cstride, int dx_accumulate,
                      float *dw1, float *dw2 /* both may be NULL */, int accumulate_w, int N, int H, int W, int C,
                      float *gate_out /* fp32 [N][C], may be NULL */, void *workspace, size_t workspace_bytes, void *stream);


/* ------------------------------------------------------------------------------------------------
 * Training step of the conv block -- replaces autograd + cuDNN/ATen for nn.Conv2d / nn.BatchNorm2d (batch
 * statistics) / nn.PReLU under loss.backward() (train.py:268-282, model/models.py:49-66).
 *
 *   forward   z = conv(x, W) [+ bias]            ryolo_conv2d_bn_act_stats with scale = 1, shift = bias|0, act linear;
 *                                                with stat_part it also emits partial sums of z and z^2 per channel.
 *                                                STATISTICS REQUIRE shift == 0 (a BatchNorm conv has no bias): the rows of
 *                                                the last pixel tile past N*Ho*Wo are summed too, and they are exact zeros
 *                                                only then; a bias conv needs no statistics and passes stat_part = NULL
 *             mean, invstd, scale, shift         ryolo_bn_finalize (biased variance, eps; running stats with momentum)
 *             y = act(z*scale + shift) [+ res]   ryolo_bn_act_fwd
 *   backward  dz, dgamma, dbeta, dslope          ryolo_bn_act_bwd   (dz = scale*(g - mean(g) - xhat*mean(g*xhat)))
 *             dx (+)= conv^T(dz, W)              ryolo_conv2d_dgrad (stride 1: flipped filter; stride 2: 4 parity classes)
 *             dW  += sum_pix dz (x) x            ryolo_conv2d_wgrad (MFMA over pixels, split-K, fp32 partial tiles)
 */
/* Layer 0 (3x3 / stride 1 / pad 1, 3 -> 32 channels on the 8-channel padded NHWC input; ryolo_conv0_recompute_supported) trains
 * WITHOUT its conv output: z0 is four times the size of x and costs 27 MACs per value, so the engine recomputes it instead of
 * storing and re-reading it (4.9 GB less HBM traffic per bs-64 step):
 *   statistics            ryolo_conv2d_bn_act_stats with y = NULL (sums only; scale = 1, shift = 0)  ->  ryolo_bn_finalize
 *   y = act(BN(z0))       ryolo_conv0_bn_act_fwd   (batch statistics folded into scale / shift; `slope`: device scalar, PReLU)
 *   dz0, dgamma, ...      ryolo_conv0_bn_bwd       (reduce pass and apply pass both recompute z0 from x; same arguments and results
 *                                                   as ryolo_bn_act_bwd on the stored z0; workspace zeroed by the caller or
 *                                                   workspace_is_zero = 0; it is left zeroed)
 * Replaces nn.Conv2d + nn.BatchNorm2d + nn.PReLU of module_list[0] under autograd (model/models.py:49-66). */
int ryolo_conv0_recompute_supported(const ryolo_conv_desc *desc);
int ryolo_conv0_bn_act_fwd(const ryolo_conv_desc *desc, const void *x, const void *w_packed, const float *scale, const float *shift,
                           int act, const float *slope, void *y, void *stream);
size_t ryolo_conv0_bn_bwd_workspace_bytes(void);
int ryolo_conv0_bn_bwd(const ryolo_conv_desc *desc, const void *x, const void *w_packed, const void *dy, int dy_cstride,
                       const float *scale, const float *shift, const float *mean, const float *invstd, int act, const float *slope,
                       void *dz, int dz_cstride, float *dgamma, float *dbeta, float *dslope, void *workspace, size_t workspace_bytes,
                       int workspace_is_zero, void *stream);
/* Layer 0's WHOLE backward in one pass over dy (csrc/conv0_bwd.hip): the weight gradient of a layer without a data gradient is linear
 * in dz, so dz = scale * (g - S1/M - xhat * S2/M) never has to exist --
 *     dW[co][k] = scale_co * (G - (S1/M) Sx - (S2 invstd / M) (Z - mean Sx)),  G = sum_p g x, Z = sum_p z x, Sx = sum_p x
 * and one kernel that recomputes z from x accumulates S1, S2, S3 (slope), G, Z, Sx; two small kernels finish.  Replaces
 * ryolo_conv0_bn_bwd + ryolo_conv2d_wgrad for that layer (8.6 GB -> 1.9 GB of traffic at bs 64 / 608^2).  dgamma / dbeta / dslope are
 * accumulated into, grad_oihw ([32][cin_real][3][3] fp32) accumulated into or overwritten; workspace: any contents.  Partial rows
 * are per workgroup and summed in a fixed order: bit-reproducible.  Autograd of /root/reference/model/models.py:49-66, layer 0. */
size_t ryolo_conv0_bn_bwd_wgrad_workspace_bytes(void);
int ryolo_conv0_bn_bwd_wgrad(const ryolo_conv_desc *desc, const void *x, const void *w_packed, const void *dy, int dy_cstride,
                             const float *scale, const float *shift, const float *mean, const float *invstd, int act, const float *slope,
                             float *dgamma, float *dbeta, float *dslope, float *grad_oihw, int cin_real, int accumulate, void *workspace,
                             size_t workspace_bytes, void *stream);
int ryolo_conv_stat_rows(const ryolo_conv_desc *desc);
int ryolo_conv2d_bn_act_stats(const ryolo_conv_desc *desc, const void *x, const void *w_packed, const float *scale,
                              const float *shift, const void *residual, void *y,
                              double *stat_part /* fp64 [ryolo_conv_stat_rows][2][cpad(Cout)], ZEROED by the caller, or NULL */,
                              void *stream);
/* ryolo_bn_finalize reads the partial sums of channels [0, C) and writes zeros back over them, so one scratch buffer
 * that starts zeroed can serve every conv of a step without a memset per layer. */
int ryolo_bn_finalize(double *stat_part, int rows, int cpad, int C, long long count, float eps, float momentum,
                      const float *gamma, const float *beta, float *mean, float *invstd, float *scale, float *shift,
                      float *running_mean /* may be NULL */, float *running_var, void *stream);
int ryolo_bn_act_fwd(const void *z, int z_cstride, const float *scale, const float *shift, int act,
                     const float *slope /* device scalar or NULL */, const void *residual, int res_cstride, void *y,
                     int y_cstride, long long npix, int C, void *stream);
size_t ryolo_bn_act_bwd_workspace_bytes(long long npix, int C);
int ryolo_bn_act_bwd(const void *z, int z_cstride, const void *dy, int dy_cstride, const float *scale, const float *shift,
                     const float *mean, const float *invstd, int act, const float *slope, void *dz, int dz_cstride,
                     long long npix, int C, float *dgamma, float *dbeta, float *dslope, void *workspace,
                     size_t workspace_bytes, void *stream);
size_t ryolo_conv_packed_dgrad_bytes(int Cout, int Cin, int ksize, int stride);
int ryolo_conv_dgrad_tap_table(int ksize, int stride, int *host_out /* host int[72] */);
int ryolo_conv_pack_weights_dgrad(const float *w_oihw, int Cout, int Cin, int ksize, int stride, void *packed,
                                  const int *taps_table /* device int[72], a copy of ryolo_conv_dgrad_tap_table's output */,
                                  void *stream);
int ryolo_conv2d_dgrad(const ryolo_conv_desc *forward_desc, const void *dz, int dz_cstride, const void *packed_dgrad,
                       const float *ones, const float *zeros /* fp32 [cpad(Cin)] */, void *dx, int accumulate, void *stream);
/* The first pass of a block's BatchNorm / activation backward folded into the launch that PRODUCES its dy (autograd runs them as
 * separate ops: model/models.py:61-62 is a BatchNorm2d node, :281-282 the shortcut add whose gradient feeds it).  In a residual
 * chain the final gradient of a 3x3 block's output is written by the data gradient of the NEXT block's 1x1 conv (accumulating into
 * the chain's running gradient); ryolo_conv2d_dgrad_bnreduce is that data gradient and additionally reads the 3x3 block's conv
 * output z and leaves the per-channel partial sums of ryolo_bn_act_bwd's reduce pass in `part` ([rows][3][C_in] fp32, any
 * contents on entry), so that ryolo_bn_act_bwd_reduced only has to finalise and apply: the 3x3 block's z and dy are read once
 * less per step.  Activation leaky / PReLU only.  Kernels that carry the reduce: for 1x1 stride-1 layers with whole 128-channel
 * tiles the persistent 2x2 tile or conv_pw.hip (one row of `part` per workgroup); for the stride-1 layers whose plain data gradient
 * runs on a one-tile-per-workgroup tile (3x3 with C_in <= 128: the 128 x 128 and 256 x 64 tiles) that tile (one row per pixel tile;
 * ryolo_bn_act_bwd_reduced folds more than 2048 rows to 64 before it finalises -- workspace >= (3 + 192) * C floats for that).
 * ryolo_conv2d_dgrad_bnreduce_rows: 0 = this conv's data gradient cannot carry the reduce (stride 2, a layer conv_mq / conv_mp
 * or the persistent narrow tiles serve, ragged channel tiles ...) -- use the two separate calls; otherwise the rows of `part`. */
int ryolo_conv2d_dgrad_bnreduce_rows(const ryolo_conv_desc *forward_desc);
int ryolo_conv2d_dgrad_bnreduce(const ryolo_conv_desc *forward_desc, const void *dz, int dz_cstride, const void *packed_dgrad,
                                const float *ones, const float *zeros, void *dx, int accumulate,
                                const void *z /* conv output of the block that produced this conv's input */, int z_cstride,
                                const float *scale, const float *shift, const float *mean, const float *invstd /* its BatchNorm */,
                                const float *slope /* device scalar */, float *part /* [rows][3][C_in] */, void *stream);
int ryolo_bn_act_bwd_reduced(const void *z, int z_cstride, const void *dy, int dy_cstride, const float *scale, const float *shift,
                             const float *mean, const float *invstd, int act /* RYOLO_ACT_LEAKY */, const float *slope, void *dz,
                             int dz_cstride, long long npix, int C, float *dgamma, float *dbeta, float *dslope, const float *part,
                             int rows, void *workspace /* 3*C floats */, size_t workspace_bytes, void *stream);
size_t ryolo_conv_wgrad_workspace_bytes(const ryolo_conv_desc *forward_desc);
/* (measurement) the two launches of ryolo_conv2d_wgrad as separate calls -- the tile kernel that writes the split-K partials, then the
 * reduce into grad_oihw -- so that a caller bracketing calls with events times them apart.  Same arguments; partials then reduce ==
 * ryolo_conv2d_wgrad. */
int ryolo_conv2d_wgrad_partials(const ryolo_conv_desc *forward_desc, const void *x, const void *dz, int dz_cstride, int Cin_real,
                                float *grad_oihw, int accumulate, void *workspace, size_t workspace_bytes, void *stream);
int ryolo_conv2d_wgrad_reduce(const ryolo_conv_desc *forward_desc, const void *x, const void *dz, int dz_cstride, int Cin_real,
                              float *grad_oihw, int accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* All split-K reduces of a backward segment as ONE launch (round 5).  ryolo_conv2d_wgrad_partials leaves a layer's partial tiles in ITS OWN
 * workspace (ryolo_conv_wgrad_workspace_bytes each; they must all stay alive until the batch has run); ryolo_conv_wgrad_reduce_job_fill
 * describes the reduce ryolo_conv2d_wgrad_reduce would launch for that layer as one job (returns its block count, 0 on a bad argument); the
 * caller lays the jobs out back to back (block_begin / block_end running sums), uploads the table once and calls
 * ryolo_conv_wgrad_reduce_batch(device_jobs, njobs, total_blocks) where the gradients are due -- the same bits as the per-layer reduces.
 * Replaces: autograd's per-layer weight-gradient accumulation behind /root/reference/train.py:268-282. */
typedef struct ryolo_wgrad_reduce_job {
    const float *part;   /* the layer's partial tiles [S][Cout_pad][Kpad] (device) */
    float *g;            /* fp32 OIHW gradient (device) */
    int S, Cout, Cin_real, Cin_k, ks, Kpad, Cout_pad, accumulate;
    int kind;            /* 0 one element per thread, 1 four split quarters per workgroup, 2 transposing 3x3 variant, 3 = 1 with four
                            input channels per thread and a quarter's loads all in flight, 4 = 2 with every load of a workgroup in flight (3, 4: the
                            batched launch's own forms, the same bits as 1 and 2) */
    int block_begin, block_end;
    int wide;            /* kinds 3, 4: several four-channel groups / (c_out, 64 c_in) units per workgroup (set by job_fill; 0 = one) */
} ryolo_wgrad_reduce_job;
int ryolo_conv_wgrad_reduce_job_fill(ryolo_wgrad_reduce_job *host_job, const ryolo_conv_desc *forward_desc, int Cin_real, const void *workspace,
                                     float *grad_oihw, int accumulate);
int ryolo_conv_wgrad_reduce_batch(const ryolo_wgrad_reduce_job *device_jobs, int njobs, int total_blocks, void *stream);
int ryolo_conv2d_wgrad(const ryolo_conv_desc *forward_desc, const void *x, const void *dz, int dz_cstride, int Cin_real,
                       float *grad_oihw /* fp32 [Cout][Cin_real][k][k] */, int accumulate, void *workspace,
                       size_t workspace_bytes, void *stream);
int ryolo_upsample2x_bwd(const void *dy, int dy_cstride, void *dx, int dx_cstride, int N, int H, int W, int C,
                         int accumulate, void *stream);
int ryolo_pgrad_to_nhwc(const float *pgrad, int bs, int na, int ny, int nx, int no, void *out, int out_cstride,
                        void *stream);

/* All weight packs of a training step in one launch.  A job packs one layout of one conv's fp32 OIHW weights:
 * kind 0 = the forward layout of ryolo_conv_pack_weights, kind 1 = one class of ryolo_conv_pack_weights_dgrad, kind 2 = one
 * x-fused stride-2 class (3x3 stride-2 convs with C_in in {32, 64}: two extra images behind the four classic ones, used by
 * ryolo_conv2d_dgrad when the input gradient is dense and its width even -- both column parities in one launch).
 * ryolo_conv_pack_job_fill (host) writes the 1 + (0 | 1 | 4 | 6) jobs of a conv into host_jobs (room for 7) and returns how many; the
 * caller concatenates all convs' jobs, turns each job's [0, block_end) into a running [block_begin, block_end) range,
 * uploads the array once and calls ryolo_conv_pack_batch(device_jobs, njobs, total_blocks) every step. */
typedef struct ryolo_pack_job {
    const void *src;   /* fp32 OIHW weights (device) */
    void *dst;         /* packed bf16 destination (device) */
    int kind, Cout, Cin, KS, Cin_pad, ntaps, Kpad, rows;
    int khs[9], kws[9];
    int block_begin, block_end;
} ryolo_pack_job;
int ryolo_conv_pack_job_fill(ryolo_pack_job *host_jobs, const float *w_oihw, int Cout, int Cin, int ksize, int stride,
                             int Cin_pad, void *packed_fwd, void *packed_dgrad);
int ryolo_conv_pack_batch(const ryolo_pack_job *device_jobs, int njobs, int total_blocks, void *stream);

/* ---------------------------------------------------------------------------------------------- training loss
 * One head of compute_loss (model/loss.py:266-367, 'default' arcs) and its gradient, no host synchronisation:
 *   lobj  = obj * mean_cells BCE(p[...,5], tobj; pos_weight obj_pw)                       (loss.py:346-348, all cells)
 *   lreg  = reg * (mean SmoothL1(sigmoid(p_xy), t_xy) + 2 mean SmoothL1(atan(p_a) + anchor_a, t_a)
 *                  + giou * mean(1 - wh_iou(t_wh, min(exp(p_wh), 1e3) * anchor_wh)))       (loss.py:314-323)
 *   lcls  = cls * mean BCE(p[...,6:], onehot; pos_weight cls_pw)          when nc > 1      (loss.py:329-333)
 * over the candidates (a, t) of the [na, NT] grid with w[a*NT + t] > 0 (build_targets, loss.py:161-258, in the
 * fixed-shape form of model/loss_static.py).  Per target t: image b, cell (gj, gi), class, cell offset txy, size twh and
 * angle ta in grid units.  npos = device scalar sum(w).  items[0..2] (lobj, lcls, lreg, already weighted) are
 * ACCUMULATED (the caller zeroes them once for all heads); dp [same shape as p] is overwritten with d(loss)/dp.
 * bitmap: ryolo_yolo_loss_bitmap_bytes(bs*na*ny*nx) bytes, zeroed by the caller (one bit per cell: several candidates
 * may share a cell, its objectness target is set once).  fp32; sums by atomics (order not fixed).                      */
/* build_targets (model/loss.py:161-258) over padded targets, all heads in one launch, no host synchronisation.
 * tpad [NT,7] rows (img, cls, x, y, w, h, angle) normalised, valid [NT] u8.  Per head h (host arrays of device pointers):
 * ng[h] = float[2] grid size (nx, ny), anchor_vec[h] = float[na,3]; outputs w[h] float[na,NT] (1 = positive candidate),
 * idx[h] int64[4,NT] = (image, class, gj, gi), box[h] float[5*NT] = txy [NT,2] | twh [NT,2] | ta [NT] in grid units (the
 * arrays ryolo_yolo_loss takes),
 * npos[h] float[1] (zeroed by the caller) += number of positives.  Every quirk of the reference is kept (cumulative
 * context rescale per head, angle gate on the last head's anchors, first-maximum / smallest-angle fallback). */
#define RYOLO_MAX_HEADS 4
int ryolo_build_targets(const float *tpad, const unsigned char *valid, int NT, int nheads, int na, const float *const *ng,
                        const float *const *anchor_vec, float iou_t, float ang_t, float context_factor, float *const *w,
                        long long *const *idx, float *const *box, float *const *npos, void *stream);
size_t ryolo_yolo_loss_bitmap_bytes(long long cells);
int ryolo_yolo_loss(const float *p, int bs, int na, int ny, int nx, int no, int nc, const float *w, int NT,
                    const long long *b, const long long *gj, const long long *gi, const long long *cls, const float *txy,
                    const float *twh, const float *ta, const float *anchor_vec /* [na,3] */, const float *npos, float giou,
                    float reg_w, float cls_w, float cls_pw, float obj_w, float obj_pw,
                    int iou_mode /* 0: wh_iou (reference, loss.py:322); 1: rotated IoU of the decoded box (riou) */,
                    unsigned *bitmap, float *dp, float *items /* [>=3] */, void *stream);

/* The same loss for a head that lives in the training engine: reads the head the conv wrote (`head`, bf16 NHWC, channel =
 * a*no + k; `p` is its fp32 [bs,na,ny,nx,no] copy, gathered by the positives) and writes d(loss)/d(head) as bf16 NHWC
 * (`head_grad`) -- the layout the head conv's backward consumes -- instead of an fp32 dp + a layout pass.  dp_sparse: fp32
 * [bs,na,ny,nx,no], ALL ZERO on entry and on exit (scratch for the positives' atomics; touched cells are re-zeroed).
 * bitmap as above (zeroed by the caller).  C = na*no and both channel strides must be multiples of 8. */
int ryolo_yolo_loss_nhwc(const void *head, int head_cstride, const float *p, int bs, int na, int ny, int nx, int no, int nc,
                         const float *w, int NT, const long long *b, const long long *gj, const long long *gi,
                         const long long *cls, const float *txy, const float *twh, const float *ta, const float *anchor_vec,
                         const float *npos, float giou, float reg_w, float cls_w, float cls_pw, float obj_w, float obj_pw,
                         int iou_mode, unsigned *bitmap, float *dp_sparse, void *head_grad, int head_grad_cstride, float *items,
                         void *stream);
/* buf[npix][C] (bf16, pixel stride cstride) *= g[0] unless g[0] == 1: the upstream gradient of loss.backward() applied to a
 * head gradient produced at loss time; returns after one scalar load in the usual g == 1 case. */
/* The other arcs of compute_loss (model/loss.py:284-286 focal wrappers -- the reference's usage note train.py:380 is
 * `--arc Fdefault` --, :350-360 unified heads, model/models.py:210-218): the same two functions with
 *   arc      RYOLO_ARC_FOCAL (every criterion but the IoU term is wrapped: loss *= (1.000001 - exp(-loss))^fl_gamma per element)
 *            | at most one of RYOLO_ARC_UBCE (BCE over the class logits of all cells, mean over cells*nc, in items[0]; no separate
 *            objectness / class-at-positives terms) and RYOLO_ARC_UCE (cross entropy over (background, classes) = logits 5..5+nc of
 *            all cells, mean over cells, in items[1]);  arc = 0 is the 'default' arc of the functions above;
 *   bitmap   ryolo_yolo_loss_bitmap_bytes_arc(cells, nc, arc) bytes, zeroed by the caller (uBCE keeps one more bit per (cell, class)).
 * no <= 32 for arc != 0. */
#define RYOLO_ARC_FOCAL 1
#define RYOLO_ARC_UBCE 2
#define RYOLO_ARC_UCE 4
size_t ryolo_yolo_loss_bitmap_bytes_arc(long long cells, int nc, int arc);
int ryolo_yolo_loss_arc(const float *p, int bs, int na, int ny, int nx, int no, int nc, const float *w, int NT,
                        const long long *b, const long long *gj, const long long *gi, const long long *cls, const float *txy,
                        const float *twh, const float *ta, const float *anchor_vec, const float *npos, float giou, float reg_w,
                        float cls_w, float cls_pw, float obj_w, float obj_pw, int iou_mode, int arc, float fl_gamma, unsigned *bitmap,
                        float *dp, float *items, void *stream);
int ryolo_yolo_loss_nhwc_arc(const void *head, int head_cstride, const float *p, int bs, int na, int ny, int nx, int no, int nc,
                             const float *w, int NT, const long long *b, const long long *gj, const long long *gi,
                             const long long *cls, const float *txy, const float *twh, const float *ta, const float *anchor_vec,
                             const float *npos, float giou, float reg_w, float cls_w, float cls_pw, float obj_w, float obj_pw,
                             int iou_mode, int arc, float fl_gamma, unsigned *bitmap, float *dp_sparse, void *head_grad,
                             int head_grad_cstride, float *items, void *stream);
int ryolo_scale_bf16_if(const float *g, void *buf, int cstride, long long npix, int C, void *stream);
/* The head conv's bias gradient out of the loss's dense pass ('default' arc, C = na*no <= 512).  ryolo_yolo_loss_nhwc_bias is
 * ryolo_yolo_loss_nhwc_arc whose dense kernel also sums, per channel, the bf16 head-gradient values it stores (the positives merged)
 * and writes rows of partial sums: bias_part [ryolo_yolo_loss_bias_rows(...)][bias_cstride] fp32, C <= bias_cstride <= 512, a multiple
 * of 8; every row is written, the buffer needs no clearing.  bias_part NULL: exactly ryolo_yolo_loss_nhwc_arc.  The rows query returns 0
 * where the fold is not served.  head_grad is byte-identical with and without bias_part.
 * ryolo_head_bias_finalize (npix = bs*ny*nx): dbias[c] += g[0] * sum over rows.  Rows and finalize add in the order of ryolo_bn_act_bwd's
 * bias form (scale == NULL) over the head gradient -- ryolo_bn_act_bwd_bias_order: its slabs and pixel lanes; a row is one pixel lane of
 * one slab -- so for g[0] == 1 dbias receives the same bits (no atomics anywhere).  g: the device scalar of the upstream gradient (the
 * rows hold the unscaled sums; the separate pass sums the values ryolo_scale_bf16_if scaled and rounded: equal for powers of two).
 * workspace: ryolo_head_bias_workspace_bytes(npix, C). */
int ryolo_bn_act_bwd_bias_order(long long npix, int C, long long *slab_pixels, int *pixel_lanes);   /* returns the number of slabs */
int ryolo_yolo_loss_bias_rows(int bs, int na, int ny, int nx, int no, int arc);
int ryolo_yolo_loss_nhwc_bias(const void *head, int head_cstride, const float *p, int bs, int na, int ny, int nx, int no, int nc,
                              const float *w, int NT, const long long *b, const long long *gj, const long long *gi,
                              const long long *cls, const float *txy, const float *twh, const float *ta, const float *anchor_vec,
                              const float *npos, float giou, float reg_w, float cls_w, float cls_pw, float obj_w, float obj_pw,
                              int iou_mode, int arc, float fl_gamma, unsigned *bitmap, float *dp_sparse, void *head_grad,
                              int head_grad_cstride, float *items, float *bias_part, int bias_cstride, void *stream);
size_t ryolo_head_bias_workspace_bytes(long long npix, int C);
int ryolo_head_bias_finalize(const float *bias_part, long long npix, int bias_cstride, int C, const float *g, float *dbias, void *workspace,
                             size_t workspace_bytes, void *stream);

/* Rotated IoU of n box pairs (cx, cy, w, h, angle; angle convention of get_rotated_coors, utils/utils.py:702-725) and its
 * gradient with respect to the FIRST box: iou [n], grad [n,5] (may be NULL).  The value is the polygon IoU of
 * skewiou (utils/utils.py:663-699) in fp32 (IoU(A, A) = 1); the reference has no backward for it -- this is the kernel of
 * the build's `riou` loss (hyp['riou'] = 1: lreg's wh_iou term becomes giou * mean(1 - riou(pbox, tbox))).
 * One pair per lane, boundary-integral form (csrc/riou_grad.h).  Degenerate boxes (w or h <= 0): 0, zero gradient. */
int ryolo_riou_loss_pairs(const float *pbox, const float *tbox, int n, float *iou, float *grad, void *stream);

/* ---------------------------------------------------------------------------------------------- optimizer
 * The SGD step of train.py:70-83 (momentum, nesterov, per-group weight decay) for every parameter tensor in one launch.
 * jobs: device array, one per tensor (fp32 p / grad / momentum buffer, n elements, param-group index, `first` = the
 * momentum buffer is uninitialised (first step: buf = d), [block_begin, block_end) = its workgroup range);
 * group_hparams: device float[groups][4] = (lr, momentum, weight_decay, gradient scale; 0 = no scaling -- data-parallel
 * runs pass 1/world instead of dividing the all-reduced gradient in a separate pass).  Same arithmetic as torch.optim.SGD. */
typedef struct ryolo_sgd_job {
    void *p;
    const void *g;
    void *buf;
    long long n;
    int group, first, block_begin, block_end;
} ryolo_sgd_job;
int ryolo_sgd_step(const ryolo_sgd_job *device_jobs, int njobs, int total_blocks, const float *group_hparams, int nesterov,
                   void *stream);

/* The Adam step of train.py:77-82 (`--adam`: torch.optim.Adam, amsgrad = maximize = False, L2 weight decay per group) for every
 * parameter tensor in one launch.  jobs: device array, one per tensor that has a gradient (fp32 p / grad / exp_avg / exp_avg_sq,
 * n elements, `row` = its row of the table below, [block_begin, block_end) = its workgroup range, ascending and gap-free over
 * the jobs; total_blocks = the last block_end).  A tensor whose four pointers are 16-byte aligned moves 16 bytes per lane, any
 * other 4 (gradients that are views into a flat bucket); both give the same bits.
 * rows: device float[rows][8] = (step_size = -lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), 1 - beta1, beta2, 1 - beta2, eps,
 * weight_decay, gradient scale; 0 = no scaling, as in ryolo_sgd_step), computed by the caller in doubles and rounded to fp32.
 * One row per (param group, step count t): torch counts steps per parameter, and one that had no gradient for a while lags behind.
 * Per element, in torch.optim.Adam's operator order and fp32 (IEEE sqrt and divide, no contraction):
 *   d = g (* scale) (+ weight_decay * p);  m += (1 - beta1) * (d - m);  v = v * beta2 + ((1 - beta2) * d) * d;
 *   p += step_size * (m / (sqrt(v) / bc2_sqrt + eps)).
 * Only enqueues.  RYOLO_EINVAL: a null table or njobs / total_blocks <= 0. */
typedef struct ryolo_adam_job {
    void *p;
    const void *g;
    void *m;
    void *v;
    long long n;
    int row, block_begin, block_end;
} ryolo_adam_job;
int ryolo_adam_step(const ryolo_adam_job *device_jobs, int njobs, int total_blocks, const float *rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RYOLO_H */
