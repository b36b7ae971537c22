"""the depth-frame preprocessing in front of the encoder, on the device.

The reference does this on the host with OpenCV for every camera message and every environment step
(``env_lab.py``: ``listener_callback`` :420-434, ``add_nose`` :78-89, ``blurring`` :69-76, ``get_center_band`` :33-39,
``cv2.resize(..., (160, 128))`` and ``/ 255`` :295-299 / :348-349).  Here the frames stay in HBM as fp32 ``(B, H, W)``
(or ``(H, W)``) tensors and every stage is a HIP kernel of ``libdgvit_hip.so``; function names follow the reference.
Parity against OpenCV itself is unpinned (cv2 is not installed in the build image; see oracle/dgvit_oracle.py f4_*).
"""
import ctypes
import numbers

import torch

from . import _lib
from .functional import _dev, _ptr, _seed_args, _stream


def _frames(img):
    img = _dev(img, "image")
    if img.dim() == 2:
        return img.unsqueeze(0), True
    if img.dim() != 3:
        raise _lib.DgvitError(f"image must be (H, W) or (B, H, W), got {tuple(img.shape)}")
    return img, False


def get_center_band(image):
    """(y1, y2) of the horizontal centre band of height H // 5 (env_lab.py:33-39)."""
    h = image.shape[-2]
    band = h // 5
    y1 = h // 2 - band // 2
    return y1, y1 + band


def depth_to_uint8(depth):
    """float depth -> 0..255 integers (``cv2.normalize(..., 0, 255, NORM_MINMAX).astype(np.uint8)``, env_lab.py:424-426), kept as fp32."""
    lib = _lib.load()
    x, squeeze = _frames(depth)
    B, H, W = x.shape
    out = torch.empty_like(x)
    scratch = torch.empty(128 * B, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.dgvit_depth_normalize_u8(_ptr(x), _ptr(out), _ptr(scratch), scratch.numel(), B, H, W, _stream()), "dgvit_depth_normalize_u8")
    return out[0] if squeeze else out


def _blur(x, ksize, y0, y1):
    lib = _lib.load()
    B, H, W = x.shape
    out = x.clone()
    tmp = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.dgvit_gaussian_blur(_ptr(x), _ptr(out), _ptr(tmp), B, H, W, ksize, y0, y1, _stream()), "dgvit_gaussian_blur")
    return out


def add_nose(image, noise_level=0.02, noise=None, seed=None):
    """``clip(image + N(0, noise_level), 0, 255)`` then a 5x5 Gaussian blur (env_lab.py:78-89).  ``noise``: the draw to add (same
    shape; parity tests); otherwise it is drawn on the device from ``seed`` (default: torch's CPU generator)."""
    lib = _lib.load()
    x, squeeze = _frames(image)
    B, H, W = x.shape
    if x.numel() % 4:
        raise _lib.DgvitError("add_nose: the number of pixels must be a multiple of 4")
    if noise is not None:
        noise = _dev(noise, "noise").reshape(x.shape)
    elif seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(lib.dgvit_noise_clip(_ptr(x), _ptr(noise), _ptr(y), x.numel(), float(noise_level), int(seed or 0), _stream()), "dgvit_noise_clip")
    out = _blur(y, 5, 0, H)
    return out[0] if squeeze else out


def blurring(image):
    """11x11 Gaussian blur of the horizontal centre band (env_lab.py:69-76)."""
    x, squeeze = _frames(image)
    y1, y2 = get_center_band(x)
    out = _blur(x, 11, y1, y2)
    return out[0] if squeeze else out


def resize_state(image, size=(128, 160)):
    """``cv2.resize(image, (160, 128)) / 255`` (env_lab.py:295,299 and :348-349); ``size`` = (height, width)."""
    lib = _lib.load()
    x, squeeze = _frames(image)
    B, H, W = x.shape
    out = torch.empty(B, size[0], size[1], dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.dgvit_resize_bilinear(_ptr(x), _ptr(out), B, H, W, size[0], size[1], 1.0 / 255.0, _stream()), "dgvit_resize_bilinear")
    return out[0] if squeeze else out


def depth_to_state(depth, noise_level=50, noise=None, seed=None, size=(128, 160)):
    """The whole chain of the reference in one call: listener_callback (normalise -> uint8 -> add_nose(50) -> blurring) followed by
    the resize + /255 of ``step`` / ``reset``: depth ``(B, H, W)`` -> encoder frames ``(B, size[0], size[1])`` in [0, 1]."""
    lib = _lib.load()
    x, squeeze = _frames(depth)
    B, H, W = x.shape
    if noise is not None:
        noise = _dev(noise, "noise").reshape(x.shape)
    elif seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    n = lib.dgvit_depth_preprocess_scratch_floats(B, H, W)
    scratch = torch.empty(n, dtype=torch.float32, device=x.device)
    state = torch.empty(B, size[0], size[1], dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.dgvit_depth_to_state(_ptr(x), _ptr(noise), float(noise_level), int(seed or 0), _ptr(state), _ptr(scratch), n, B, H, W,
                                      size[0], size[1], _stream())
    _lib.check(rc, "dgvit_depth_to_state")
    return state[0] if squeeze else state


# ------------------------------------------------------------------------------------------------ random shift (DrQ), DESIGN.md 3.24
def _shift_pad(pad, shape, what="pad"):
    """``pad`` as an int after the checks every random-shift caller shares; host-only, runs before anything touches a device"""
    if isinstance(pad, bool) or not isinstance(pad, numbers.Integral):
        raise ValueError(f"{what} must be an integer number of pixels, got {pad!r}")
    if pad < 0:
        raise ValueError(f"{what} must be >= 0, got {pad}")
    if pad == 0:
        return 0
    if len(shape) != 2:
        raise ValueError(f"{what}: frames must be (H, W), got {tuple(shape)}")
    if pad >= min(shape):
        raise ValueError(f"{what}={pad} must be smaller than the frame's shorter side (H, W) = {tuple(shape)}")
    return int(pad)


def _shift_seed(device):
    """The seed of one shifted batch, drawn as GoT.draw_dropout_seed() draws the dropout seed: an int from torch's CPU generator, or,
    inside a stream capture, a 1-element int64 device tensor (a host value would be frozen into every replay)."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(1, dtype=torch.int64, device=device).random_()
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _gather_shift(src, idx, out, shifts, frame, nrows, pad, stream_id, seed):
    """dgvit_gather_shift_frames, or its _u8 form for a uint8 src, on the current stream (the caller has made src's device current): out
    (B, row) fp32 <- rows ``idx`` (None: 0..B-1) of src (nrows, src.shape[1]), each shifted by its own draw; ``seed`` is an int or a
    1-element int64 device tensor; ``shifts`` (B, 2) int32 or None receives (dy, dx)."""
    seed_val, seed_dev = _seed_args(seed)
    name, row_bytes = ("dgvit_gather_shift_frames_u8", (src.shape[1],)) if src.dtype == torch.uint8 else ("dgvit_gather_shift_frames", ())
    rc = getattr(_lib.load(), name)(_ptr(src), _ptr(idx), _ptr(out), _ptr(shifts), out.shape[0], frame[0], frame[1], *row_bytes,
                                    out.shape[1], nrows, pad, stream_id, seed_val, _ptr(seed_dev), _stream())
    _lib.check(rc, name)


def random_shift(frames, pad, seed=None, stream_id=0, return_shifts=False):
    """DrQ random shift of a batch that does not come from ``DeviceReplayBuffer`` (e.g. a behaviour-cloning loader): every frame of
    ``frames`` (B, H, W) is padded by ``pad`` pixels with its border (``F.pad(mode="replicate")``) and cropped back at its own offset
    (pad + dy, pad + dx), dy and dx uniform in [-pad, pad].  One kernel, one read and one write per pixel; the result is a new tensor.
    ``seed`` (int, or a 1-element int64 device tensor for graph capture; default: drawn from torch's CPU generator) and ``stream_id``
    fix the draw (include/dgvit_hip.h: dgvit_gather_shift_frames); ``return_shifts`` adds the (B, 2) int32 table of (dy, dx)."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"frames: expected a tensor, got {type(frames).__name__}")
    if frames.dim() != 3:
        raise _lib.DgvitError(f"frames must be (B, H, W), got {tuple(frames.shape)}")
    B, H, W = frames.shape
    pad = _shift_pad(pad, (H, W))
    x = _dev(frames, "frames").reshape(B, H * W)
    row = (H * W + 3) & ~3
    if row != H * W:                       # the kernel reads and writes rows of whole float4 groups
        src = x.new_zeros(B, row)
        src[:, :H * W] = x
    else:
        src = x if x.data_ptr() % 16 == 0 else x.clone()
    out = torch.empty(B, row, dtype=torch.float32, device=x.device)
    shifts = torch.empty(B, 2, dtype=torch.int32, device=x.device) if return_shifts else None
    with torch.cuda.device(x.device):
        _gather_shift(src, None, out, shifts, (H, W), B, pad, int(stream_id), _shift_seed(x.device) if seed is None else seed)
    res = out[:, :H * W].reshape(B, H, W)
    return (res, shifts) if return_shifts else res
