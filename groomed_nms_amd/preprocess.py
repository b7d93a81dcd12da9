"""The image front end of the reference's loop on the GPU (lib/augmentations.py; csrc/preprocess.hip): what turns the
uint8 BGR images cv2.imread gives into the float32 RGB planes the network reads.

  preprocess_images   a batch of uint8 HWC BGR images of any sizes -> float32 [B, 3, H, W] on the device in ONE launch
                      (gnms_preprocess_images): mirror, bilinear resize to size[0] rows, crop / zero-pad to size[1] columns, x / 255,
                      - mean, / std, BGR -> RGB planes.  Host images are packed into one reused pinned buffer, table first, and go
                      up with one copy; a device buffer plus table is read where it lies (stream-ordered, graph-capturable).
  Preprocess          lib/augmentations.py:410-438 with its constructor arguments; __call__(img) -> device tensor [3, h, w].
                      detect.im_detect_3d takes a tensor from `preprocess` as it is.
  Augmentation        lib/augmentations.py:376-407 for a batch: __call__(images, imobjs) -> (tensor [B, 3, H, W], imobjs), followed by
                      the RGB swap and transpose of lib/imdb_util.py:522-526.  Per image one np.random.rand() <= mirror_prob, drawn
                      in image order as the reference's Compose draws it, so a run seeded like the reference's mirrors the same images.
                      The imobj side (RandomMirror.flip_gts, ego_mirror, Resize.scale_gts, imobj.scale_factor) stays on the host in
                      float64 with the reference's expressions in the reference's order: bit for bit the reference's.

Supported: three channels, uint8, scale factors size[0] / H >= 1 (the shipped configs' 512 / 375), distort_prob <= 0; anything else
raises NotImplementedError.  There is no CPU implementation of the image path here.
"""
import ctypes
import logging
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

__all__ = ["preprocess_images", "Preprocess", "Augmentation", "describe", "resized_width", "ego_mirror", "flip_gts", "scale_gts", "DESC"]

DESC = 5                                             # GNMS_PREPROCESS_DESC: offset, H, W, width after the resize, mirror
_ALIGN = 256                                         # of the image region and of every image inside the packed buffer
_GT_KEYS = ("gts", "gts_1", "gts_2", "gts_3")
_EGO_KEYS = ("ego_32", "ego_31", "ego_30", "ego_21", "ego_20", "ego_10")


def _size(size):
    size = list(size) if isinstance(size, (list, tuple, np.ndarray)) else [size]
    if len(size) not in (1, 2) or any(int(s) != s or s < 1 for s in size):
        raise ValueError("size must be [height] or [height, width] in whole pixels, got %r" % (size,))
    return [int(s) for s in size]


def resized_width(H, W, size0):
    """Resize.__call__ (:88-91): (scale_factor, w) of an H x W image brought to size0 rows; np.round rounds half to even"""
    scale_factor = size0 / H
    h = int(np.round(H * scale_factor).astype(int))
    w = int(np.round(W * scale_factor).astype(int))
    if h != size0:                                   # H * (size0 / H) is within an ulp of size0
        raise ValueError("an image of %d rows does not resize to %d rows (np.round gives %d)" % (H, size0, h))
    return scale_factor, w


def describe(shapes, size, mirror=None):
    """The descriptor table of a batch, on the host: shapes [(H, W, 3), ...] -> (table int64 [B, 5] with the offsets of the images laid
    one after the other, each at a multiple of 256 bytes; total bytes; H_out; W_out).  Raises what preprocess_images raises for sizes."""
    size = _size(size)
    B = len(shapes)
    flags = [False] * B if mirror is None else [bool(m) for m in mirror]
    if len(flags) != B:
        raise ValueError("mirror has %d entries for %d images" % (len(flags), B))
    table = np.zeros((B, DESC), np.int64)
    off = 0
    for i, shp in enumerate(shapes):
        if len(shp) != 3:
            raise ValueError("image %d: shape %r, expected [H, W, 3]" % (i, tuple(shp)))
        H, W, C = (int(s) for s in shp)
        if C != 3:
            raise NotImplementedError("image %d has %d channels; only three-channel (single-frame BGR) images are implemented" % (i, C))
        if H < 1 or W < 1:
            raise ValueError("image %d is empty: %r" % (i, tuple(shp)))
        scale_factor, w = resized_width(H, W, size[0])
        if scale_factor < 1:
            raise NotImplementedError("image %d: scale factor %d / %d < 1 (reduction) is not implemented" % (i, size[0], H))
        table[i] = (off, H, W, w, int(flags[i]))
        off += -(-H * W * 3 // _ALIGN) * _ALIGN
    if len(size) > 1:
        W_out = size[1]
    else:
        widths = sorted(set(int(w) for w in table[:, 3]))
        if len(widths) > 1:
            raise ValueError("a one-element size leaves the width to the images, and they resize to different widths %r: "
                             "give size [height, width]" % (widths,))
        W_out = widths[0] if widths else 1
    return table, off, size[0], W_out


def _device(device):
    if not torch.cuda.is_available():
        raise _lib.GnmsError("needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    dev = torch.device("cuda" if device is None else device)
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _norm(image_means, image_stds):
    mean = np.array(image_means, dtype=np.float32).reshape(-1)                        # Normalize.__init__ (:46-48)
    stds = np.array(image_stds, dtype=np.float32).reshape(-1)
    if mean.shape[0] != 3 or stds.shape[0] != 3:
        raise ValueError("image_means / image_stds must have three entries each, got %d / %d" % (mean.shape[0], stds.shape[0]))
    return (ctypes.c_float * 3)(*mean.tolist()), (ctypes.c_float * 3)(*stds.tolist())


class _Pinned:
    """one pinned staging buffer per device, grown as needed; the event says when the last copy out of it has finished"""
    buffers = {}

    @classmethod
    def get(cls, dev, nbytes):
        buf, event = cls.buffers.get(dev, (None, None))
        if event is not None:
            event.synchronize()                      # the previous batch has left the buffer
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty((max(nbytes, 1 << 20),), dtype=torch.uint8).pin_memory()
        cls.buffers[dev] = (buf, event)
        return buf

    @classmethod
    def copied(cls, dev, buf):
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(dev))
        cls.buffers[dev] = (buf, event)


def _upload(images, table, nbytes, dev):
    """host images + table -> (device buffer of the images, device table) through the pinned buffer with one copy"""
    B = len(images)
    head = -(-B * DESC * 8 // _ALIGN) * _ALIGN
    pinned = _Pinned.get(dev, head + nbytes)
    host = pinned.numpy()
    host[:B * DESC * 8] = table.reshape(-1).view(np.uint8)
    for img, row in zip(images, table):
        n = int(row[1] * row[2] * 3)
        host[head + int(row[0]):head + int(row[0]) + n] = img.reshape(-1)
    staged = torch.empty((head + nbytes,), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        staged.copy_(pinned[:head + nbytes], non_blocking=True)
        _Pinned.copied(dev, pinned)
    return staged[head:], staged[:B * DESC * 8].view(torch.int64).view(B, DESC)


def _launch(buffer, table, B, H_out, W_out, image_means, image_stds, dev):
    mean, stds = _norm(image_means, image_stds)
    out = torch.empty((B, 3, H_out, W_out), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        check(_lib.load().gnms_preprocess_images(ptr(buffer), buffer.numel(), ptr(table), B, H_out, W_out, mean, stds, ptr(out), stream_ptr(dev)),
              "gnms_preprocess_images")
    return out


def preprocess_images(images, size, image_means, image_stds, mirror=None, device=None):
    """-> float32 [B, 3, size[0], W] on the device, RGB planes, normalised with image_means / image_stds in the reference's order (entry
    0 on the blue channel).  W = size[1], or with a one-element size the common width the images resize to.

    images: a list of uint8 [H, W, 3] BGR ndarrays or tensors (all on the host, or all on the device), sizes free per image, with
            mirror = None or one flag per image; or a pair (buffer, table) already on the device -- a uint8 tensor and an int64 [B, 5]
            table of (byte offset, H, W, width after the resize, mirror) as `describe` lays it out -- with a two-element size and
            mirror = None (the flags are in the table).  That path reads nothing on the host: it is stream-ordered and can be captured;
            the caller answers for the table (an image that does not lie inside the buffer is left unwritten)."""
    size = _size(size)
    _norm(image_means, image_stds)
    if isinstance(images, tuple) and len(images) == 2 and torch.is_tensor(images[0]) and torch.is_tensor(images[1]) and images[1].dtype == torch.int64:
        buffer, table = images
        dev = _device(device)
        if mirror is not None:
            raise ValueError("with a device buffer and table the mirror flags are the table's fifth column")
        if len(size) != 2:
            raise ValueError("with a device buffer and table, size must be [height, width]")
        if buffer.dtype != torch.uint8 or buffer.device != dev or table.device != dev or not buffer.is_contiguous() or not table.is_contiguous():
            raise ValueError("buffer (uint8) and table (int64) must be contiguous tensors on %s" % (dev,))
        if table.dim() != 2 or table.shape[1] != DESC:
            raise ValueError("table must be [B, %d], got %s" % (DESC, tuple(table.shape)))
        return _launch(buffer, table, table.shape[0], size[0], size[1], image_means, image_stds, dev)
    images = list(images)
    for i, img in enumerate(images):
        if not (torch.is_tensor(img) or isinstance(img, np.ndarray)):
            raise TypeError("image %d is a %s; expected a uint8 ndarray or tensor" % (i, type(img).__name__))
        if img.dtype != (torch.uint8 if torch.is_tensor(img) else np.uint8):
            raise TypeError("image %d is %s; the front end reads uint8 images (cv2.imread's)" % (i, img.dtype))
    table, nbytes, H_out, W_out = describe([tuple(img.shape) for img in images], size, mirror)
    dev = _device(device)                            # after the argument checks: they need no GPU
    B = len(images)
    if B == 0:
        return torch.empty((0, 3, H_out, W_out), dtype=torch.float32, device=dev)
    on_device = [torch.is_tensor(img) and img.is_cuda for img in images]
    if all(on_device):
        buffer = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
        for img, row in zip(images, table):
            buffer[int(row[0]):int(row[0]) + img.numel()] = img.to(dev).reshape(-1)
        table_dev = torch.from_numpy(table).to(dev)
    elif any(on_device):
        raise ValueError("the images must be all on the host or all on the device")
    else:
        host = [np.ascontiguousarray(img.numpy() if torch.is_tensor(img) else img) for img in images]
        buffer, table_dev = _upload(host, table, nbytes, dev)
    return _launch(buffer, table_dev, B, H_out, W_out, image_means, image_stds, dev)


class Preprocess(object):
    """lib/augmentations.py:410-438 (ConvertToFloat, Resize, Normalize, RGB swap, transpose) on the GPU: __call__(img) -> device tensor
    [3, h, w] float32."""

    def __init__(self, size, mean, stds, device=None):
        self.mean = mean
        self.stds = stds
        self.size = size
        self.device = device
        _size(size)
        _norm(mean, stds)

    def __call__(self, img):
        return preprocess_images([img], self.size, self.mean, self.stds, device=self.device)[0]


# ---------------------------------------------------------------------------------------------------- the imobj side (host, float64)
def ego_mirror(ego):
    """lib/util.py:411-425"""
    pose_dx, pose_dy, pose_dz, pose_rx, pose_ry, pose_rz = ego
    pose_dx *= -1
    pose_ry *= -1
    pose_rz *= -1
    while pose_ry > math.pi: pose_ry -= math.pi * 2          # noqa: E701
    while pose_ry < (-math.pi): pose_ry += math.pi * 2       # noqa: E701
    while pose_rz > math.pi: pose_rz -= math.pi * 2          # noqa: E701
    while pose_rz < (-math.pi): pose_rz += math.pi * 2       # noqa: E701
    return [pose_dx, pose_dy, pose_dz, pose_rx, pose_ry, pose_rz]


def _rot_to_alpha(ry3d, z3d, x3d):
    """convertRot2Alpha, the scalar branch (lib/util.py:673-677)"""
    alpha = ry3d - math.atan2(-z3d, x3d) - 0.5 * math.pi
    while alpha > math.pi: alpha -= math.pi * 2              # noqa: E701
    while alpha <= (-math.pi): alpha += math.pi * 2          # noqa: E701
    return alpha


def _snap_to_pi(ry3d):
    """snap_to_pi, the scalar branch (lib/math_3d.py:507-508)"""
    while ry3d > math.pi: ry3d -= math.pi * 2                # noqa: E701
    while ry3d <= (-math.pi): ry3d += math.pi * 2            # noqa: E701
    return ry3d


def flip_gts(width, imobj, key):
    """RandomMirror.flip_gts (:217-279) with image.shape[1] = width, the width BEFORE the resize: the reference's expressions in the
    reference's order on the reference's types, so every float64 comes out the same."""
    for gtind, gt in enumerate(imobj[key]):
        if "bbox_full" in gt:
            gt["bbox_full"][0] = width - gt["bbox_full"][0] - gt["bbox_full"][2]
        if "bbox_vis" in gt:
            gt["bbox_vis"][0] = width - gt["bbox_vis"][0] - gt["bbox_vis"][2]
        if "bbox_3d" in gt:
            gt["bbox_3d"][0] = width - gt["bbox_3d"][0] - 1
            rotY = gt["bbox_3d"][10]
            rotY = (-math.pi - rotY) if rotY < 0 else (math.pi - rotY)
            while rotY > math.pi: rotY -= math.pi * 2        # noqa: E701
            while rotY < (-math.pi): rotY += math.pi * 2     # noqa: E701
            cx2d = gt["bbox_3d"][0]
            cy2d = gt["bbox_3d"][1]
            cz2d = gt["bbox_3d"][2]
            coord3d = imobj["p2_inv"].dot(np.array([cx2d * cz2d, cy2d * cz2d, cz2d, 1]))
            alpha = _rot_to_alpha(rotY, coord3d[2], coord3d[0])
            axis_lbl = np.abs(np.sin(alpha)) < np.abs(np.cos(alpha))
            alpha_sin = alpha
            alpha_cos = alpha
            while alpha_sin > (math.pi / 2): alpha_sin -= math.pi        # noqa: E701
            while alpha_sin <= (-math.pi / 2): alpha_sin += math.pi      # noqa: E701
            while alpha_cos > (0): alpha_cos -= math.pi                  # noqa: E701
            while alpha_cos <= (-math.pi): alpha_cos += math.pi          # noqa: E701
            pick = alpha_sin if axis_lbl == 1 else alpha_cos
            both = [np.abs(pick - alpha), np.abs(_snap_to_pi(pick + math.pi) - alpha)]
            head_acc = np.min(both)
            head_lbl = np.argmin(both)
            if not np.isclose(head_acc, 0):
                logging.warning("WARNING, error in heading calculation not accurate!")
            gt["bbox_3d"][10] = rotY
            gt["bbox_3d"][6] = alpha
            gt["bbox_3d"][12] = alpha_sin
            gt["bbox_3d"][13] = alpha_cos
            gt["bbox_3d"][14] = axis_lbl
            gt["bbox_3d"][15] = head_lbl
            gt["bbox_3d"][7:10] = coord3d[:3]
            gt["center_3d"] = coord3d[:3]


def scale_gts(imobj, scale_factor, key):
    """Resize.scale_gts (:69-83)"""
    for gt in imobj[key]:
        if "bbox_full" in gt:
            gt["bbox_full"] *= scale_factor
        if "bbox_vis" in gt:
            gt["bbox_vis"] *= scale_factor
        if "bbox_3d" in gt:
            gt["bbox_3d"][0] *= scale_factor                 # only the 2D centre
            gt["bbox_3d"][1] *= scale_factor


class Augmentation(object):
    """lib/augmentations.py:376-407 for a batch.  conf: image_means, image_stds, crop_size, mirror_prob, distort_prob (<= 0).
    __call__(images, imobjs) -> (float32 [B, 3, H, W] on the device, imobjs); the imobjs (dict-like, as easydict's; None for an image
    without one) are changed in place as the reference changes them."""

    def __init__(self, conf, device=None):
        self.mean = conf["image_means"]
        self.stds = conf["image_stds"]
        self.size = conf["crop_size"]
        self.mirror_prob = conf["mirror_prob"]
        self.distort_prob = conf["distort_prob"]
        self.device = device
        if self.distort_prob > 0:
            raise NotImplementedError("Augmentation: distort_prob=%r > 0 (the photometric distortion, torchvision's ColorJitter) is not implemented"
                                      % (self.distort_prob,))
        _size(self.size)
        _norm(self.mean, self.stds)

    def host_pass(self, shapes, imobjs):
        """What the reference's Compose does per image apart from the pixels, in image order: the draw of RandomMirror (:286, one
        np.random.rand() per image), ego_mirror and flip_gts when it mirrors, then Resize's scale_factor and scale_gts (:107-115).
        shapes: the images' (H, W, 3) before the resize.  -> the mirror flags."""
        size = _size(self.size)
        if len(shapes) != len(imobjs):
            raise ValueError("%d images, %d imobjs" % (len(shapes), len(imobjs)))
        flags = []
        for shp, imobj in zip(shapes, imobjs):
            H, width = int(shp[0]), int(shp[1])
            mirrored = bool(np.random.rand() <= self.mirror_prob)
            flags.append(mirrored)
            if mirrored and imobj:
                for key in _EGO_KEYS:
                    if key in imobj:
                        imobj[key] = ego_mirror(imobj[key])
                for key in _GT_KEYS:
                    if key in imobj:
                        flip_gts(width, imobj, key)
            if imobj:
                scale_factor = size[0] / H
                imobj["scale_factor"] = scale_factor
                for key in _GT_KEYS:
                    if key in imobj:
                        scale_gts(imobj, scale_factor, key)
        return flags

    def __call__(self, images, imobjs):
        images = list(images)
        shapes = [tuple(img.shape) for img in images]
        describe(shapes, self.size)                          # what cannot be done raises before a draw is made or an imobj changed
        flags = self.host_pass(shapes, imobjs)
        return preprocess_images(images, self.size, self.mean, self.stds, mirror=flags, device=self.device), imobjs
