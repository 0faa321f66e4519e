"""NHWC8Batch: a batch of images already in the engines' input layout -- bf16 [N, H, W, 8], channels 3..7 zero, what
ryolo_nchw_f32_to_nhwc_bf16 makes of an fp32 [N, 3, H, W] tensor.  Darknet.forward, HipEngine and TrainEngine.forward accept it in
place of the fp32 NCHW tensor and skip the converter; the ATen chain converts it back with ryolo_nhwc_bf16_to_nchw_f32 (float())."""
import torch


class NHWC8Batch(object):
    def __init__(self, data, channels=3):
        if not (torch.is_tensor(data) and data.dim() == 4 and data.shape[3] == 8 and data.dtype == torch.bfloat16 and data.is_contiguous()):
            raise ValueError("NHWC8Batch wants a contiguous bf16 [N, H, W, 8] tensor")
        if not data.is_cuda:
            raise RuntimeError("NHWC8Batch lives on a GPU device: the layout is the HIP engines' input, there is no CPU path")
        if not 1 <= channels <= 8:
            raise ValueError("channels must be 1..8")
        self.data = data
        self.channels = int(channels)

    @property
    def shape(self):
        """the logical NCHW shape"""
        n, h, w, _ = self.data.shape
        return torch.Size((n, self.channels, h, w))

    device = property(lambda self: self.data.device)
    dtype = property(lambda self: self.data.dtype)
    is_cuda = True

    def __len__(self):
        return self.data.shape[0]

    def to(self, device):
        """the batch on another GPU (itself when it is there already).  Only the device can change: the layout fixes the dtype."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError("NHWC8Batch cannot move to %s: there is no CPU path (float() gives the fp32 NCHW tensor)" % device)
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        return self if device == self.data.device else NHWC8Batch(self.data.to(device), self.channels)

    def float(self):
        """fp32 [N, C, H, W]: the values an fp32 loader would have handed over, after the engines' own bf16 rounding"""
        from . import hip_ops
        return hip_ops.nhwc_bf16_to_nchw_f32(self.data[..., :self.channels])

    def copy_into(self, x_nhwc):
        """Put the batch into an engine's input buffer (bf16 [N, H, W, 8] view): a device-to-device copy on the current stream, or
        nothing when the batch IS that buffer.  Returns whether a copy was enqueued."""
        if tuple(x_nhwc.shape) != tuple(self.data.shape) or x_nhwc.device != self.data.device:
            raise RuntimeError("engine was planned for an NHWC8Batch of %s on %s, not %s on %s"
                               % (tuple(x_nhwc.shape), x_nhwc.device, tuple(self.data.shape), self.data.device))
        if self.data.data_ptr() == x_nhwc.data_ptr() and self.data.stride() == x_nhwc.stride():
            return False
        x_nhwc.copy_(self.data)
        return True
