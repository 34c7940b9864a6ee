"""vp8g_stage -- what every device-call wrapper of vp8g.py does around its call, once.

  Source       the source byte image: every array off its alignment by a chosen shift, pad bytes between
  Guarded      a destination or work buffer with guard bytes around its regions, and the check that they survived
  device_copy  host descriptors to the device
  call         the ctypes call: tensors to pointers, the error texts, the EINVAL path of the entry points' checks
  file_spans, scale_opts, batch_flags, take_images   the arguments and results of the end-to-end (file-level) calls

Source and Guarded are numpy only (tests/test_stage.py holds their layouts to tests/golden/stage_layout.json without
a GPU); torch is imported where a function touches the device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

PAD = 0x5A  # the byte between and behind sources: a kernel that reads it as data shows in the comparison
BATCH_DEVICE_M05, BATCH_MULTI_PARTITION = 1, 2  # VP8G_BATCH_*


class ByteSpan(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("size", C.c_size_t)]


class Source:
    """The source bytes of one launch.  `placed` lists (offset, align, shift) of every array."""

    def __init__(self):
        self.buf, self.placed = bytearray(), []

    def put(self, array, align: int = 1, shift: int = 0) -> int:
        """Pad up to `align`, then `shift` bytes more, then the array's bytes: their offset."""
        self.buf += bytes([PAD]) * ((-len(self.buf)) % align + shift)
        self.placed.append((len(self.buf), align, shift))
        self.buf += np.ascontiguousarray(array).tobytes()
        return self.placed[-1][0]

    def reserve(self, nbytes: int, align: int = 1) -> int:
        """Room for bytes whose content depends on their own offset (`fill` them later)."""
        return self.put(np.zeros(nbytes, np.uint8), align)

    def fill(self, offset: int, data: bytes):
        self.buf[offset:offset + len(data)] = data

    def finish(self, tail: int = 16) -> np.ndarray:
        return np.frombuffer(self.buf + bytes([PAD]) * tail, np.uint8)


class Guarded:
    """A buffer of `fill` bytes: `head` exempt bytes, then `guard` bytes in front of, between and behind the regions,
    each region rounded up to `round_to`.  `regions` lists (offset, nbytes); `size` is the whole buffer."""

    def __init__(self, guard: int, fill: int, round_to: int = 1, head: int = 0):
        self.guard, self.fill, self.round_to, self.head = guard, fill, round_to, head
        self.size, self.regions = head + guard, []

    def add(self, nbytes: int) -> int:
        self.regions.append((self.size, nbytes))
        self.size += -(-nbytes // self.round_to) * self.round_to + self.guard
        return self.regions[-1][0]

    def check(self, host: np.ndarray, what: str):
        """AssertionError("<what> were written") unless every byte outside the regions (and the head) is `fill`."""
        keep = np.ones(self.size, bool)
        keep[:self.head] = False
        for o, n in self.regions:
            keep[o:o + n] = False
        if host.shape != keep.shape or not (host[keep] == self.fill).all():
            raise AssertionError(f"{what} were written")

    def on_device(self):
        import torch
        return torch.full((self.size,), self.fill, dtype=torch.uint8, device=device())

    def fetch(self, tensor, what: str):
        """The buffer back on the host as a torch CPU tensor, once checked."""
        host = tensor.cpu()
        self.check(host.numpy(), what)
        return host


def device():
    import torch
    return torch.device("cuda", 0)


def stream():
    import torch
    return torch.cuda.current_stream(device())


def upload(array: np.ndarray):
    import torch
    return torch.from_numpy(array).to(device())


def device_copy(c_array, tail: int = 0, dev=None):
    """The uint8 device tensor that holds a ctypes array's (or structure's) bytes and `tail` zero bytes."""
    import torch
    return torch.frombuffer(bytearray(bytes(c_array)) + bytearray(tail), dtype=torch.uint8).to(dev or device())


def call(lib, name: str, *args, einval=None, untouched=None):
    """lib.<name>(*args) with torch tensors and (tensor, byte shift) pairs as pointers.  A non-zero return raises
    RuntimeError; with einval=ValueError an EINVAL refusal raises that instead, after untouched=(tensor, fill) is seen
    to hold `fill` still."""
    def ptr(a):
        t, shift = a if isinstance(a, tuple) else (a, 0)
        return C.c_void_p(t.data_ptr() + shift) if hasattr(t, "data_ptr") else a

    if getattr(lib, name)(*[ptr(a) for a in args]) == 0:
        return
    en = C.get_errno()
    if einval is not None and en == 22:
        if untouched is not None:
            import torch
            torch.cuda.synchronize()
            if not bool((untouched[0] == untouched[1]).all()):
                raise AssertionError(f"{name}: a refused call wrote to the output")
        raise einval(f"{name}: EINVAL")
    raise RuntimeError(f"{name} failed: errno={en} {lib.vp8g_last_error()!r}")


def file_spans(files):
    """(buffers to keep alive, ByteSpan array) of a list of byte strings."""
    bufs = [(C.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0") for b in files]
    return bufs, (ByteSpan * len(files))(*[ByteSpan(C.cast(buf, C.POINTER(C.c_uint8)), len(b)) for buf, b in zip(bufs, files)])


def scale_opts(scale):
    """(ctypes array or None, count) of scale = None, one Vp8gScaleOpt for every file, or a list of one per file."""
    opts = [] if scale is None else (list(scale) if isinstance(scale, (list, tuple)) else [scale])
    return ((type(opts[0]) * len(opts))(*opts) if opts else None), len(opts)


def batch_flags(device_m05: bool, multi_partition: bool) -> int:
    return (BATCH_DEVICE_M05 if device_m05 else 0) | (BATCH_MULTI_PARTITION if multi_partition else 0)


def image_bytes(img) -> bytes:
    ysz = img.stride_y * img.height
    uvsz = img.stride_uv * ((img.height + 1) // 2)
    return C.string_at(img.y, ysz) + C.string_at(img.u, uvsz) + C.string_at(img.v, uvsz)


def take_images(lib, imgs, st, with_size: bool):
    """The Yuv420Images of an end-to-end call as I420 bytes -- (bytes, w, h) if with_size -- or None where st is not 0;
    every image is freed."""
    out = []
    for img, s in zip(imgs, st):
        b = image_bytes(img) if s == 0 else None
        out.append((b, int(img.width), int(img.height)) if with_size and s == 0 else b)
        lib.yuv420_free(C.byref(img))
    return out
