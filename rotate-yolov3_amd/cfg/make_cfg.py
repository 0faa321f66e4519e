"""Generate Darknet .cfg text for the rotated-YOLOv3 topologies this build benchmarks.

The reference ships its cfgs as hand-edited copies of stock darknet files; the two BASELINE.json names
(cfg/yolov3.cfg, cfg/yolov3-tiny.cfg) do not even load in its own parser.  Here the same
topologies are produced by code so that width/height/anchors/classes are parameters:

  darknet53(...)   Darknet-53 trunk + 3-scale FPN head, 75 convs / 23 shortcuts / 4 routes / 2 upsamples / 3 yolo
                   (layer indices as SURVEY.md Appendix A: yolo at 82, 94, 106; routes 83, 86, 95, 98)
  darknet53_se(...)  the same with a squeeze-and-excitation block in front of every residual unit of the 256 / 512 / 1024
                   stages (the reference's cfg/ICDAR/yolov3_608_se.cfg and cfg/HRSC+/yolov3_512_se.cfg): 127 layers, 20 se
  darknet53_matrix(...)  Darknet-53 + FPN plus the "matrix" heads of the reference's cfg/HRSC+/yolov3_512_matrix.cfg: a stride-64 head
                   behind layer 79 and, per FPN level (layers 74 / 86 / 98), one branch per dilation that re-uses the weights of that
                   level's head convs (weight_from) with its 3x3 convs dilated ([d-convolutional]); 16 yolo layers by default
  tiny(...)        yolov3-tiny: 13 convs, 6 maxpools, 2 yolo heads

    python -m rotate_yolov3_amd.cfg.make_cfg darknet53 > yolov3.cfg
"""
import sys

ANCHORS_ARA = ("792, 2061, 3870, 6353, 9623, 15803 / 4.18, 6.48, 8.71  / "
               "-75, -60, -45, -30, -15 ,0,15, 30,45, 60,75, 90")   # the values of the reference's cfg/yolov3.cfg:609
TINY_PAIRS = "10,14,  23,27,  37,58,  81,82,  135,169,  344,319"


def _net(width, height):
    return ["[net]", "batch=16", "subdivisions=1", "width=%d" % width, "height=%d" % height, "channels=3", ""]


def _conv(filters, size, stride, bn=1, act="leaky"):
    out = ["[convolutional]"]
    if bn:
        out.append("batch_normalize=1")
    out += ["filters=%d" % filters, "size=%d" % size, "stride=%d" % stride, "pad=1", "activation=%s" % act, ""]
    return out


def _yolo(mask, anchors, classes):
    return ["[yolo]", "mask = %s" % mask, "anchors = %s" % anchors, "classes=%d" % classes, "num=9", ""]


def darknet53(width=608, height=608, anchors="ara " + ANCHORS_ARA, classes=1, na_per_head=72, masks=None, se=False):
    """se=True: [se] + conv 1x1 + conv 3x3 + shortcut from=-4 in the 256 / 512 / 1024 stages (the skip comes from in front of the se);
    the absolute route indices 61 and 36 stay as they are and then name shortcut layers inside the 38^2 and 76^2 stages"""
    no = na_per_head * (classes + 6)
    masks = masks or ["%d-%d" % (2 * na_per_head, 3 * na_per_head - 1), "%d-%d" % (na_per_head, 2 * na_per_head - 1),
                      "0-%d" % (na_per_head - 1)]
    L = _net(width, height)
    L += _conv(32, 3, 1)
    for filters, nblocks in ((64, 1), (128, 2), (256, 8), (512, 8), (1024, 4)):
        L += _conv(filters, 3, 2)
        for _ in range(nblocks):
            if se and filters >= 256:
                L += ["[se]", "channels=%d" % filters, ""]
            L += _conv(filters // 2, 1, 1) + _conv(filters, 3, 1)
            L += ["[shortcut]", "from=%d" % (-4 if se and filters >= 256 else -3), "activation=linear", ""]
    # head 0 @ stride 32
    for _ in range(3):
        L += _conv(512, 1, 1) + _conv(1024, 3, 1)
    L += _conv(no, 1, 1, bn=0, act="linear") + _yolo(masks[0], anchors, classes)
    # head 1 @ stride 16
    L += ["[route]", "layers = -4", ""] + _conv(256, 1, 1) + ["[upsample]", "stride=2", ""]
    L += ["[route]", "layers = -1, 61", ""]
    for _ in range(3):
        L += _conv(256, 1, 1) + _conv(512, 3, 1)
    L += _conv(no, 1, 1, bn=0, act="linear") + _yolo(masks[1], anchors, classes)
    # head 2 @ stride 8
    L += ["[route]", "layers = -4", ""] + _conv(128, 1, 1) + ["[upsample]", "stride=2", ""]
    L += ["[route]", "layers = -1, 36", ""]
    for _ in range(3):
        L += _conv(128, 1, 1) + _conv(256, 3, 1)
    L += _conv(no, 1, 1, bn=0, act="linear") + _yolo(masks[2], anchors, classes)
    return "\n".join(L) + "\n"


def darknet53_se(width=608, height=608, anchors="ara " + ANCHORS_ARA, classes=1, na_per_head=72, masks=None):
    """the topology of the reference's cfg/ICDAR/yolov3_608_se.cfg: se blocks at layers 13, 17, ..., 41, 46, ..., 74, 79, ..., 91"""
    return darknet53(width, height, anchors, classes, na_per_head, masks, se=True)


MATRIX_DILATIONS = (((1, 2), (2, 1)),                                             # branches off layer 74 (stride 32)
                    ((1, 2), (2, 1), (1, 4), (4, 1)),                             # layer 86 (stride 16)
                    ((1, 2), (2, 1), (1, 4), (4, 1), (1, 8), (8, 1)))             # layer 98 (stride 8)


def _shared(kind, filters, size, weight_from, bn=1, act="leaky", dilation=None):
    out = ["[%s]" % kind]
    if dilation is not None:
        out.append("dilation=(%d,%d)" % tuple(dilation))
    if bn:
        out.append("batch_normalize=1")
    return out + ["filters=%d" % filters, "size=%d" % size, "stride=1", "pad=1", "activation=%s" % act, "weight_from = %d" % weight_from, ""]


def darknet53_matrix(width=512, height=512, anchors="ara " + ANCHORS_ARA, classes=1, na_per_head=72, dilations=MATRIX_DILATIONS):
    """the layer graph of the reference's cfg/HRSC+/yolov3_512_matrix.cfg: layers 0-106 are darknet53(); 107-111 the stride-64 head
    (route 79, 3x3 / 2, 1x1 with bias, head, yolo); then per level l (source layer 74 / 86 / 98, head convs l+1 .. l+7) and per dilation
    one branch of 11 layers: route l, 1x1 (weight_from l+1), dilated 3x3 (l+2), 1x1 (l+3), dilated 3x3 (l+4), shortcut -3, 1x1 (l+5),
    dilated 3x3 (l+6), shortcut -3, head 1x1 (l+7), yolo.  Every branch of a level uses that level's anchor mask, the stride-64 head the
    stride-32 one; one dilation per branch (the shipped file mixes (2,1) and (1,2) inside its second branch)."""
    no = na_per_head * (classes + 6)
    masks = ["%d-%d" % (2 * na_per_head, 3 * na_per_head - 1), "%d-%d" % (na_per_head, 2 * na_per_head - 1), "0-%d" % (na_per_head - 1)]
    L = darknet53(width, height, anchors, classes, na_per_head, masks).split("\n")[:-1]
    L += ["[route]", "layers = 79", ""] + _conv(512, 3, 2) + _conv(1024, 1, 1, bn=0) + _conv(no, 1, 1, bn=0, act="linear")
    L += _yolo(masks[0], anchors, classes)
    for level, (src, wide) in enumerate(((74, 1024), (86, 512), (98, 256))):
        for dil in dilations[level]:
            L += ["[route]", "layers = %d" % src, ""]
            for j in range(3):
                L += _shared("convolutional", wide // 2, 1, src + 1 + 2 * j)
                L += _shared("d-convolutional", wide, 3, src + 2 + 2 * j, dilation=dil)
                if j:
                    L += ["[shortcut]", "from=-3", "activation=linear", ""]
            L += _shared("convolutional", no, 1, src + 7, bn=0, act="linear") + _yolo(masks[level], anchors, classes)
    return "\n".join(L) + "\n"


def tiny(width=608, height=608, anchors=TINY_PAIRS, classes=80):
    """Stock yolov3-tiny topology with the rotated head width: stock (w,h) pairs x 12 angles, comma masks index
    pairs (3,4,5 -> anchors 36..71; 1,2,3 -> 12..47), 36 anchors per head, filters = 36*(classes+6)."""
    no = 36 * (classes + 6)
    L = _net(width, height)
    for f in (16, 32, 64, 128, 256):
        L += _conv(f, 3, 1) + ["[maxpool]", "size=2", "stride=2", ""]
    L += _conv(512, 3, 1) + ["[maxpool]", "size=2", "stride=1", ""]
    L += _conv(1024, 3, 1) + _conv(256, 1, 1) + _conv(512, 3, 1)
    L += _conv(no, 1, 1, bn=0, act="linear") + _yolo("3,4,5", anchors, classes)
    L += ["[route]", "layers = -4", ""] + _conv(128, 1, 1) + ["[upsample]", "stride=2", ""]
    L += ["[route]", "layers = -1, 8", ""] + _conv(256, 3, 1)
    L += _conv(no, 1, 1, bn=0, act="linear") + _yolo("1,2,3", anchors, classes)
    return "\n".join(L) + "\n"


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "darknet53"
    sys.stdout.write({"darknet53": darknet53, "darknet53_se": darknet53_se, "darknet53_matrix": darknet53_matrix, "tiny": tiny}[which]())
