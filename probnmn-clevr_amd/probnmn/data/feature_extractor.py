"""ResNet-101 stage-3 feature extractor on the MI355X: images -> the (1024, 14, 14) features the NMN consumes.

The reference does this offline with torchvision (``scripts/preprocess/extract_features.py:98-105``:
``resnet101(pretrained=True)`` with ``layer4`` / ``avgpool`` / ``fc`` replaced by ``nn.Identity``, eval mode; ``:124-131`` the
forward under ``no_grad``; ``:60-73`` the 224x224 resize and the normalisation) and writes an H5 file that the training
readers load back.  :class:`ResNet101Stage3` is that network with torchvision's parameter names -- a torchvision
``resnet101`` checkpoint loads with ``load_state_dict(sd, strict=False)`` (the ``layer4.*`` / ``fc.*`` keys are the ones the
reference throws away) -- running on ``libprobnmn_hip.so``: 94 launches of ``pnmn_conv2d_nhwc`` (implicit GEMM on the fp32
matrix cores; eval-mode batch norm, residual add and ReLU in the epilogue) and one max pool, NHWC throughout.  The
result is a ``channels_last`` tensor, which is the layout ``NeuralModuleNetwork`` and the feature stores
(``probnmn.data.feature_store``) take without a layout pass -- on this part the features of all 70 000 CLEVR training
images fit in HBM (56 GB of 288), so extraction can feed a ``DeviceFeatureStore`` directly instead of a file.

Decoded images go in as they are: :func:`resize_normalize` (``pnmn_image_prep``, csrc/image_prep.hip) is the transform's
``Resize((224, 224))`` -- Pillow's 8-bit bilinear resampler, integer arithmetic reproduced bit for bit -- fused with
``ToTensor`` / ``Normalize`` and the 3 -> 4 channel padding of the stem convolution's input, and
:meth:`ResNet101Stage3.forward_pixels` runs the network on its result.  Only the PNG decoding stays on the CPU.

No CPU fallback: parameters and images must be on a ROCm device.
"""
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

from probnmn import _hip

#: torchvision.models.resnet101: Bottleneck blocks per stage (the reference drops stage 4)
LAYERS = (("layer1", 64, 3, 1), ("layer2", 128, 4, 2), ("layer3", 256, 23, 2))
IMAGE_SIZE = 224            # reference extract_features.py:60-61
MEAN = (0.485, 0.456, 0.406)  # reference extract_features.py:72
STD = (0.229, 0.224, 0.224)   # (sic: the reference's third std is 0.224)


class _Bottleneck(nn.Module):
    """Parameter container with torchvision's names; the arithmetic is ResNet101Stage3.forward's."""

    def __init__(self, inplanes: int, planes: int, stride: int, downsample: bool):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, 4 * planes, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(4 * planes)
        self.stride = stride
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, stride=stride, bias=False),
                                            nn.BatchNorm2d(4 * planes))
        else:
            self.downsample = None


class _Conv:
    """One folded convolution: packed weight [Cout][Kpad], scale / shift on the device."""

    __slots__ = ("w", "scale", "shift", "cin", "cout", "k", "stride", "pad")


class ResNet101Stage3(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        for name, planes, blocks, stride in LAYERS:
            layer = []
            for b in range(blocks):
                layer.append(_Bottleneck(inplanes, planes, stride if b == 0 else 1, downsample=(b == 0)))
                inplanes = 4 * planes
            setattr(self, name, nn.Sequential(*layer))
        self.eval()
        self._packed: Optional[Dict[str, _Conv]] = None
        self._packed_key = None

    # ---- weights ------------------------------------------------------------------------------------------------
    def _fold(self, conv: nn.Conv2d, bn: nn.BatchNorm2d) -> _Conv:
        w = conv.weight.detach()
        cout, cin, kh, kw = w.shape
        cin_p = (cin + 3) // 4 * 4  # (the image: 3 -> 4 channels)
        wk = torch.zeros(cout, kh * kw, cin_p, dtype=torch.float32, device=w.device)
        wk[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
        floats = _hip.lib().pnmn_conv2d_weight_floats(cout, cin_p, kh, kw)
        if floats <= 0:
            raise _hip.HipLibraryError("pnmn_conv2d_weight_floats(%d, %d, %d, %d) = %d" % (cout, cin_p, kh, kw, floats))
        packed = torch.zeros(cout, floats // cout, dtype=torch.float32, device=w.device)
        packed[:, : kh * kw * cin_p] = wk.reshape(cout, -1)
        c = _Conv()
        scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
        c.w, c.scale, c.shift = packed, scale.float().contiguous(), (bn.bias.detach() - bn.running_mean * scale).float().contiguous()
        c.cin, c.cout, c.k, c.stride, c.pad = cin_p, cout, kh, conv.stride[0], conv.padding[0]
        return c

    def _pack(self) -> Dict[str, _Conv]:
        # (re-folded when any parameter or buffer was written: load_state_dict, .to(), an optimizer)
        key = tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))
        if self._packed is None or key != self._packed_key:
            packed = {"conv1": self._fold(self.conv1, self.bn1)}
            for name, _, blocks, _ in LAYERS:
                for b, blk in enumerate(getattr(self, name)):
                    p = "%s.%d" % (name, b)
                    packed[p + ".conv1"] = self._fold(blk.conv1, blk.bn1)
                    packed[p + ".conv2"] = self._fold(blk.conv2, blk.bn2)
                    packed[p + ".conv3"] = self._fold(blk.conv3, blk.bn3)
                    if blk.downsample is not None:
                        packed[p + ".downsample"] = self._fold(blk.downsample[0], blk.downsample[1])
            self._packed, self._packed_key = packed, key
        return self._packed

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("the extractor runs in eval mode only (reference extract_features.py:105)")
        return super().train(False)

    # ---- forward ------------------------------------------------------------------------------------------------
    @staticmethod
    def _conv(c: _Conv, x: torch.Tensor, relu: bool, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        n, h, w, cin = x.shape
        assert cin == c.cin
        ho = (h + 2 * c.pad - c.k) // c.stride + 1
        wo = (w + 2 * c.pad - c.k) // c.stride + 1
        y = torch.empty(n, ho, wo, c.cout, dtype=torch.float32, device=x.device)
        d = np.zeros(1, _hip.CONV2D_DESC)
        d[0] = (x.data_ptr(), c.w.data_ptr(), c.scale.data_ptr(), c.shift.data_ptr(),
                residual.data_ptr() if residual is not None else 0, y.data_ptr(),
                n, h, w, cin, ho, wo, c.cout, c.k, c.k, c.stride, c.pad, int(relu))
        _hip.check(_hip.lib().pnmn_conv2d_nhwc(d.ctypes.data, _hip.stream_ptr(x.device)), "conv2d_nhwc")
        return y

    @torch.no_grad()
    def forward(self, images: torch.Tensor) -> torch.Tensor:
        """``images``: (N, 3, H, W) float, normalised as the reference's transform does (:func:`preprocess`); H and W
        multiples of 32.  Returns (N, 1024, H / 16, W / 16) fp32 in ``channels_last`` memory format."""
        dev = self.conv1.weight.device
        if dev.type != "cuda" or images.device != dev:
            raise _hip.HipLibraryError("ResNet101Stage3 runs on a ROCm device only (parameters on %s, images on %s): "
                                       "there is no CPU fallback" % (dev, images.device))
        if images.dim() != 4 or images.size(1) != 3 or images.size(2) % 32 or images.size(3) % 32:
            raise ValueError("expected images (N, 3, H, W) with H and W multiples of 32, got %s" % (tuple(images.shape),))
        n, _, h, w = images.shape
        x = torch.zeros(n, h, w, 4, dtype=torch.float32, device=dev)
        x[..., :3] = images.float().permute(0, 2, 3, 1)
        return self._trunk(x)

    @torch.no_grad()
    def forward_pixels(self, images_uint8: torch.Tensor, size: Tuple[int, int] = (IMAGE_SIZE, IMAGE_SIZE)) -> torch.Tensor:
        """``images_uint8``: (N, H, W, 3) uint8 decoded RGB images of any size, on the parameters' device.  The reference's
        whole transform (``Resize(size)`` as Pillow does it, ``ToTensor``, ``Normalize``) runs in one kernel
        (:func:`resize_normalize`) whose output is the stem convolution's input; ``size`` multiples of 32.  Returns what
        :meth:`forward` returns for ``preprocess`` of the Pillow-resized images, bit for bit."""
        dev = self.conv1.weight.device
        if dev.type != "cuda" or images_uint8.device != dev:
            raise _hip.HipLibraryError("ResNet101Stage3 runs on a ROCm device only (parameters on %s, images on %s): "
                                       "there is no CPU fallback" % (dev, images_uint8.device))
        if len(size) != 2 or size[0] % 32 or size[1] % 32:
            raise ValueError("expected size (H, W) with H and W multiples of 32, got %s" % (tuple(size),))
        return self._trunk(resize_normalize(images_uint8, size))

    def _trunk(self, x: torch.Tensor) -> torch.Tensor:
        """The network on the stem convolution's input: (N, H, W, 4) fp32 NHWC, normalised, channel 3 zero."""
        dev = x.device
        packed = self._pack()
        n = x.size(0)
        x = self._conv(packed["conv1"], x, relu=True)
        pooled = torch.empty(n, x.size(1) // 2, x.size(2) // 2, 64, dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().pnmn_maxpool3x3s2_nhwc(x.data_ptr(), pooled.data_ptr(), n, x.size(1), x.size(2), 64,
                                                     _hip.stream_ptr(dev)), "maxpool3x3s2")
        x = pooled
        for name, _, blocks, _ in LAYERS:
            for b in range(blocks):
                p = "%s.%d" % (name, b)
                identity = x
                if p + ".downsample" in packed:
                    identity = self._conv(packed[p + ".downsample"], x, relu=False)
                out = self._conv(packed[p + ".conv1"], x, relu=True)
                out = self._conv(packed[p + ".conv2"], out, relu=True)
                x = self._conv(packed[p + ".conv3"], out, relu=True, residual=identity)
        return x.permute(0, 3, 1, 2)  # (N, 1024, h/16, w/16) over NHWC storage

    def flops_per_image(self, h: int = IMAGE_SIZE, w: int = IMAGE_SIZE) -> float:
        """Algorithmic FLOPs of one image (2 x MACs of the 94 convolutions; the image counted with its 3 channels)."""
        total, size, inplanes = 2.0 * (h // 2) * (w // 2) * 64 * 49 * 3, (h // 4, w // 4), 64
        for _, planes, blocks, stride in LAYERS:
            for b in range(blocks):
                s = stride if b == 0 else 1
                out_size = (size[0] // s, size[1] // s)
                total += 2.0 * size[0] * size[1] * inplanes * planes
                total += 2.0 * out_size[0] * out_size[1] * planes * planes * 9
                total += 2.0 * out_size[0] * out_size[1] * planes * 4 * planes
                if b == 0:
                    total += 2.0 * out_size[0] * out_size[1] * inplanes * 4 * planes
                size, inplanes = out_size, 4 * planes
        return total


def preprocess(images_uint8: torch.Tensor) -> torch.Tensor:
    """``ToTensor`` + ``Normalize`` of the reference's transform (extract_features.py:70-73) on (N, 3, H, W) uint8 images,
    on whatever device they are.  The transform's ``Resize((224, 224))`` (PIL, bilinear) is not in here: the images are
    already resized (:func:`resize_normalize` does all three steps on decoded images of any size)."""
    x = images_uint8.float() / 255.0
    mean = torch.tensor(MEAN, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std


@torch.no_grad()
def extract_features(model: ResNet101Stage3, image_batches: Iterable[torch.Tensor], out: torch.Tensor) -> int:
    """The reference's extraction loop (extract_features.py:124-131) into ``out`` -- (n_images, 1024, 14, 14), any device, any
    memory format: a ``channels_last`` tensor in HBM is what ``DeviceFeatureStore`` / the NMN read in place, a host tensor
    is the H5 file's content.  ``image_batches`` yields normalised (b, 3, 224, 224) batches in image order.  Returns the
    number of images written."""
    dev = model.conv1.weight.device
    counter = 0
    for batch in image_batches:
        feats = model(batch.to(dev, non_blocking=True))
        out[counter: counter + feats.size(0)].copy_(feats)
        counter += feats.size(0)
    return counter


# ---- the transform on the device: Resize (Pillow, bilinear) + ToTensor + Normalize ------------------------------------
PRECISION_BITS = 22  # Pillow's 8-bit resampler: coefficients in 32 - 8 - 2 bits of fixed point


def resize_coefficients(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's coefficient table of one axis of ``Image.resize(..., BILINEAR)`` on an 8-bit image (its
    ``precompute_coeffs`` and ``normalize_coeffs_8bpc``, in float64 as there): ``(k, bounds)`` with ``k`` int32
    [out_size][ksize] -- the taps of every output index in 22-bit fixed point, zero beyond its count -- and ``bounds``
    int32 [out_size][2] -- (first input index, number of taps).  A triangle filter whose support grows with the downscale
    factor; ``ksize = 2 * ceil(max(in / out, 1)) + 1``."""
    if in_size < 1 or out_size < 1:
        raise ValueError("resize_coefficients: sizes must be positive, got %d -> %d" % (in_size, out_size))
    scale = float(in_size) / float(out_size)
    support = max(scale, 1.0)
    ss = 1.0 / support
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    taps = np.arange(ksize, dtype=np.int64)[None, :]
    arg = ((taps + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss
    w = np.where((np.abs(arg) < 1.0) & (taps < n[:, None]), 1.0 - np.abs(arg), 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for t in range(ksize):  # (summed in tap order, as the C loop does)
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)
    return k, np.stack([xmin, n], axis=1).astype(np.int32)


def normalization_table() -> torch.Tensor:
    """fp32 [3][256]: :func:`preprocess` of every byte value per channel, so a lookup equals ``preprocess`` bit for bit."""
    values = torch.arange(256, dtype=torch.uint8).view(1, 1, 256, 1).expand(1, 3, 256, 1)
    return preprocess(values).reshape(3, 256).contiguous()


_PREP_TABLES: Dict[tuple, tuple] = {}


def _prep_tables(h: int, w: int, size: Tuple[int, int], device: torch.device) -> tuple:
    key = (h, w, int(size[0]), int(size[1]), device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _PREP_TABLES:
        (ky, yb), (kx, xb) = resize_coefficients(h, size[0]), resize_coefficients(w, size[1])
        tensors = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(device) for t in (kx, xb, ky, yb))
        _PREP_TABLES[key] = tensors + (normalization_table().to(device), kx.shape[1], ky.shape[1])
    return _PREP_TABLES[key]


def resize_normalize(images_uint8: torch.Tensor, size: Tuple[int, int] = (IMAGE_SIZE, IMAGE_SIZE)) -> torch.Tensor:
    """The reference's whole image transform (extract_features.py:60-73) on the device, in one kernel: (N, H, W, 3) uint8
    RGB images -> (N, size[0], size[1], 4) fp32 NHWC, channels 0-2 ``preprocess`` of ``PIL.Image.resize(size[::-1],
    BILINEAR)`` bit for bit, channel 3 zero -- the stem convolution's input.  The coefficient tables and the
    normalisation table are built once per (H, W, size, device)."""
    if images_uint8.dtype != torch.uint8 or images_uint8.dim() != 4 or images_uint8.size(3) != 3 or images_uint8.size(1) < 1 \
            or images_uint8.size(2) < 1:
        raise ValueError("expected uint8 images (N, H, W, 3), got %s %s" % (images_uint8.dtype, tuple(images_uint8.shape)))
    if len(size) != 2 or size[0] < 1 or size[1] < 1:
        raise ValueError("expected size (H, W), got %s" % (size,))
    if images_uint8.device.type != "cuda":
        raise _hip.HipLibraryError("resize_normalize runs on a ROCm device only (images on %s): there is no CPU fallback"
                                   % images_uint8.device)
    n, h, w, _ = images_uint8.shape
    ksy, ksx = (int(np.ceil(max(i / o, 1.0))) * 2 + 1 for i, o in ((h, size[0]), (w, size[1])))
    if max(ksx, ksy) > _hip.IMAGE_PREP_MAX_TAPS or size[1] > _hip.IMAGE_PREP_MAX_WIDTH \
            or max(h, w, size[0]) > _hip.IMAGE_PREP_MAX_SIZE:
        raise NotImplementedError(
            "resize_normalize %dx%d -> %dx%d is beyond pnmn_image_prep's limits: at most %d taps per axis (a %dx downscale; "
            "this one needs %d), output width <= %d, sizes <= %d"
            % (h, w, size[0], size[1], _hip.IMAGE_PREP_MAX_TAPS, (_hip.IMAGE_PREP_MAX_TAPS - 1) // 2, max(ksx, ksy),
               _hip.IMAGE_PREP_MAX_WIDTH, _hip.IMAGE_PREP_MAX_SIZE))
    dev = images_uint8.device
    images_uint8 = images_uint8.contiguous()
    out = torch.empty(n, size[0], size[1], 4, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    kx, xb, ky, yb, lut, ksx, ksy = _prep_tables(h, w, size, dev)
    _hip.check(_hip.lib().pnmn_image_prep(images_uint8.data_ptr(), 3 * h * w, n, h, w, kx.data_ptr(), xb.data_ptr(), ksx,
                                          ky.data_ptr(), yb.data_ptr(), ksy, lut.data_ptr(), out.data_ptr(), size[0], size[1],
                                          _hip.stream_ptr(dev)), "image_prep")
    return out


@torch.no_grad()
def extract_features_from_pixels(model: ResNet101Stage3, pixel_batches: Iterable[torch.Tensor], out: torch.Tensor,
                                 size: Tuple[int, int] = (IMAGE_SIZE, IMAGE_SIZE)) -> int:
    """:func:`extract_features` for decoded images: ``pixel_batches`` yields (b, H, W, 3) uint8 batches in image order (of
    any size; one size per batch), resized and normalised on the device (:meth:`ResNet101Stage3.forward_pixels`).
    Returns the number of images written."""
    dev = model.conv1.weight.device
    counter = 0
    for batch in pixel_batches:
        feats = model.forward_pixels(batch.to(dev, non_blocking=True), size)
        out[counter: counter + feats.size(0)].copy_(feats)
        counter += feats.size(0)
    return counter
