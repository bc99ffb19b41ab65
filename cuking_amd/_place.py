"""Where a call's arrays live.  Every feature is a pair -- ``cuking_X`` on the device and its host
twin ``cuking_X_host`` -- whose Python callers differ only in how an array is checked, allocated,
turned into a pointer and kept alive.  A place holds exactly that: ``HostPlace`` over numpy and the
host twins, ``DevicePlace`` over a ``KingContext``, an optional stream and torch.  The body of a
call (``ibd._ibd_segments_raw``, ``pcrelate._pcrelate_pairs_raw``, ...) is written once over a
place: the scalar validation, the null-pointer rules and the one argument list are in the body,
the words "array" / "tensor" / "must live on this context's GPU" are here.

``HostPlace`` never imports torch: the host twins run in processes that do not load it.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .api import KING_RESULT_DTYPE, _count, _device_tensor, _stream_handle

_PAD = np.zeros(4, dtype=np.uint64)   # the address of "nothing" where the library refuses NULL


def site_array(values, name: str, num_sites: int, dtype):
    """None, or ``values`` as a contiguous ``dtype`` ``[num_sites]`` host array."""
    if values is None:
        return None
    values = np.asarray(values)
    if values.ndim != 1 or values.shape[0] != num_sites or values.dtype.kind not in "iu":
        raise ValueError(f"{name} must be an integer [{num_sites}] array, not {values.dtype} "
                         f"{values.shape}")
    info = np.iinfo(dtype)
    if values.size and (int(values.min()) < info.min or int(values.max()) > info.max):
        raise ValueError(f"{name} must fit {np.dtype(dtype).name}")
    return np.ascontiguousarray(values, dtype=dtype)


def host_pairs(pairs, num_records=None):
    """(array that owns the memory, count, stride in bytes) of a host pair list:
    ``KING_RESULT_DTYPE`` records or ``[*, 6]`` int32 / uint32 (the first ``num_records``;
    stride 24), or an integer ``[P, 2]`` array (stride 8)."""
    pairs = np.asarray(pairs)
    if pairs.dtype == KING_RESULT_DTYPE and pairs.ndim == 1 or \
            pairs.ndim == 2 and pairs.shape[1] == 6 and pairs.dtype in (np.int32, np.uint32):
        recs = np.ascontiguousarray(pairs)
        count = recs.shape[0] if num_records is None else _count(num_records, "num_records")
        if count > recs.shape[0]:
            raise ValueError(f"pairs holds {recs.shape[0]} records, num_records is {count}")
        return recs, count, 24
    if num_records is not None:
        raise ValueError("num_records goes with a record buffer, not with a [P, 2] array")
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
        raise ValueError("pairs must be KING_RESULT_DTYPE records, [*, 6] int32 / uint32 records "
                         f"or an integer [P, 2] array, not {pairs.dtype} {pairs.shape}")
    if pairs.size and (int(pairs.min()) < 0 or int(pairs.max()) > 0xFFFFFFFF):
        raise ValueError("pairs must hold sample indices in [0, 2^32)")
    flat = np.ascontiguousarray(pairs, dtype=np.uint32)
    return flat, flat.shape[0], 8


def tensor_to_host(t, dtype) -> np.ndarray:
    """A device tensor on the host (waits for the copy): int32 ``[n, itemsize / 4]`` as ``[n]``
    rows of a structured ``dtype``, else the same shape viewed as ``dtype``."""
    host = np.ascontiguousarray(t.cpu().numpy()).view(dtype)
    return host.reshape(-1) if np.dtype(dtype).names else host


def _width(dtype) -> tuple:
    """The trailing dimension a structured ``dtype`` has as an int32 tensor."""
    return (np.dtype(dtype).itemsize // 4,) if np.dtype(dtype).names else ()


class HostPlace:
    """numpy arrays and the host twins."""

    def fn(self, name: str):
        return getattr(_lib.load(), f"cuking_{name}_host")

    def ptr(self, a, pad: bool = False):
        """The address of ``a``; None for None and for an empty array -- or, with ``pad``, the
        address of nothing, for the arguments the library refuses as NULL."""
        if a is None or not a.size:
            return _PAD.ctypes.data if pad and a is not None else None
        return a.ctypes.data

    def words(self, bits, name: str = "bits") -> int:
        assert bits.dtype == np.uint64 and bits.flags.c_contiguous, name
        return bits.size

    def bits(self, bits, words_per_sample: int) -> int:
        """The stored samples of a bitset of ``words_per_sample`` words a row."""
        return self.words(bits) // words_per_sample if words_per_sample else 0

    def sites(self, values, name: str, num_sites: int, dtype):
        return site_array(values, name, num_sites, dtype)

    def host_sites(self, values, dtype):
        return values

    def matrix(self, a, name: str, min_rows: int, cols=None):
        """``(a, leading dimension)`` of a float32 matrix whose rows are contiguous (a pitch
        between rows is fine)."""
        # (the strides of an empty array say nothing)
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or a.size and (
                (a.shape[1] > 1 and a.strides[1] != 4) or a.strides[0] % 4 or
                (a.shape[0] > 1 and a.strides[0] < 4 * a.shape[1])):
            raise ValueError(f"{name} must be a float32 [rows, cols] array with contiguous rows")
        if a.shape[0] < min_rows or cols is not None and a.shape[1] != cols:
            raise ValueError(f"{name} must have at least {min_rows} rows"
                             f"{'' if cols is None else f' of {cols} columns'}, not {a.shape}")
        return a, max(a.strides[0] // 4, a.shape[1])

    def vector(self, a, name: str, dtype, size: int):
        a = np.ascontiguousarray(a)
        if a.dtype != dtype or a.shape != (size,):
            raise ValueError(f"{name} must be {np.dtype(dtype).name} [{size}], not {a.dtype} "
                             f"{a.shape}")
        return a

    def pairs(self, pairs, num_records=None):
        return host_pairs(pairs, num_records)

    def pair_indices(self, owner, count: int, stride: int, num_stored: int) -> np.ndarray:
        """uint32 ``[count, 2]`` of what ``pairs`` returned."""
        if stride == 8:
            return owner[:count]
        if owner.dtype == KING_RESULT_DTYPE:
            return np.stack([owner["sample_i"][:count], owner["sample_j"][:count]], axis=1)
        return owner[:count, :2].view(np.uint32)

    def index_list(self, values, name: str, cols, to_host):
        return to_host(values)

    def alloc(self, shape, dtype):
        return np.zeros(shape, dtype=dtype)

    zeros = alloc

    def out(self, out, name: str, dtype, shape=None):
        assert out.dtype == dtype and out.flags.c_contiguous and \
            (shape is None or out.shape == (shape if isinstance(shape, tuple) else (shape,))), name
        return out

    def from_host(self, a, dtype=np.float32):
        return np.ascontiguousarray(a, dtype=dtype)

    def uploads_done(self):
        pass

    def keep(self, *owners):
        pass

    def finish(self):
        pass

    def trim(self, buffer, count: int):
        return buffer[:count].copy()

    def to_host(self, a, dtype, count=None):
        return a if count is None else a[:count]

    def isaf_operator(self, bits, words_per_sample: int, num_sites: int, fit):
        from .pcrelate import HostIsafOperator
        return HostIsafOperator(bits, words_per_sample, num_sites, fit)


class DevicePlace:
    """torch tensors on a ``KingContext``'s GPU and the device calls on ``stream`` (None: the
    current one).  Uploads run on the current stream: ``uploads_done()`` makes ``stream`` wait
    for them before the library call, ``keep()`` hands every copy this place made (and the
    temporaries it is given) to ``stream`` after it, because they are freed on return."""

    def __init__(self, ctx, stream=None):
        self.ctx, self.stream, self.dev = ctx, stream, f"cuda:{ctx.device}"
        self._made = []

    def fn(self, name: str):
        f, handle, stream = getattr(self.ctx.lib, f"cuking_{name}"), self.ctx.handle, self.stream
        return lambda *args: f(handle, *args, _stream_handle(stream))

    def ptr(self, a, pad: bool = False):
        if a is None or not pad and not a.numel():
            return None
        return a.data_ptr()

    def words(self, bits, name: str = "bits") -> int:
        import torch
        return _device_tensor(self.ctx.device, bits, name, torch.int64).numel()

    def bits(self, bits, words_per_sample: int) -> int:
        return self.ctx._rows_of(bits, words_per_sample)

    def _upload(self, host: np.ndarray):
        import torch
        self._made.append(torch.from_numpy(host).to(self.dev))
        return self._made[-1]

    def sites(self, values, name: str, num_sites: int, dtype):
        """As the host's, or an int32 device tensor of ``num_sites``; uint32 travels as its int32
        bit pattern."""
        import torch
        if values is None:
            return None
        if isinstance(values, torch.Tensor):
            return _device_tensor(self.ctx.device, values, name, torch.int32, shape=(num_sites,))
        return self._upload(site_array(values, name, num_sites, dtype).view(np.int32))

    def host_sites(self, values, dtype):
        import torch
        return values.cpu().numpy().view(dtype) if isinstance(values, torch.Tensor) else values

    def matrix(self, t, name: str, min_rows: int, cols=None):
        import torch
        _device_tensor(self.ctx.device, t, name, torch.float32, contiguous=False)
        # (the strides of an empty tensor say nothing)
        if t.dim() != 2 or t.numel() and ((t.shape[1] > 1 and t.stride(1) != 1) or
                                          (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
            raise ValueError(f"{name} must be a [rows, cols] tensor with contiguous rows")
        if t.shape[0] < min_rows or cols is not None and t.shape[1] != cols:
            raise ValueError(f"{name} must have at least {min_rows} rows"
                             f"{'' if cols is None else f' of {cols} columns'}, "
                             f"not {tuple(t.shape)}")
        return t, max(t.stride(0), t.shape[1])

    def vector(self, t, name: str, dtype, size: int):
        import torch
        return _device_tensor(self.ctx.device, t, name, getattr(torch, np.dtype(dtype).name),
                              shape=(size,))

    def pairs(self, pairs, num_records=None):
        """As the host's with a tensor as the owner: an int32 ``[*, 6]`` record tensor (the first
        ``num_records``), an int32 / int64 ``[P, 2]`` tensor, or one of the host forms,
        uploaded."""
        import torch
        if not isinstance(pairs, torch.Tensor):
            owner, count, stride = host_pairs(pairs, num_records)
            flat = np.ascontiguousarray(owner).view(np.int32).reshape(owner.shape[0], stride // 4)
            return self._upload(flat), count, stride
        if not pairs.is_cuda or pairs.device.index != self.ctx.device:
            raise ValueError("pairs must live on this context's GPU")
        if pairs.dim() == 2 and pairs.shape[1] == 6 and pairs.dtype == torch.int32:
            count = pairs.shape[0] if num_records is None else _count(num_records, "num_records")
            if count > pairs.shape[0]:
                raise ValueError(f"pairs holds {pairs.shape[0]} records, num_records is {count}")
            return self._own(pairs, pairs.contiguous()), count, 24
        if num_records is not None:
            raise ValueError("num_records goes with a record buffer, not with a [P, 2] tensor")
        if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype not in (torch.int32, torch.int64):
            raise ValueError("pairs must be an int32 [*, 6] record tensor or an int32 / int64 "
                             f"[P, 2] tensor, not {pairs.dtype} {tuple(pairs.shape)}")
        if pairs.dtype == torch.int64 and pairs.numel() and \
                (int(pairs.min()) < 0 or int(pairs.max()) > 0xFFFFFFFF):
            raise ValueError("pairs must hold sample indices in [0, 2^32)")
        # (int64 wraps: the low 32 bits are the uint32)
        return self._own(pairs, pairs.to(torch.int32).contiguous()), pairs.shape[0], 8

    def _own(self, given, converted):
        if converted is not given:
            self._made.append(converted)
        return converted

    def pair_indices(self, owner, count: int, stride: int, num_stored: int) -> np.ndarray:
        """As the host's, copied to the host only if an index is outside the ``num_stored``
        samples (else empty): all that a range check asks."""
        index = owner[:count, :2]
        if count and bool(((index < 0) | (index >= num_stored)).any()):   # (int32: < 0 is >= 2^31)
            return index.cpu().numpy().view(np.uint32)
        return np.zeros((0, 2), dtype=np.uint32)

    def index_list(self, values, name: str, cols, to_host):
        """An integer list (``cols`` None: ``[S]``, else ``[T, cols]``) as an int32 device tensor:
        the caller's, or ``to_host(values)`` uploaded; uint32 travels as its int32 bit pattern."""
        import torch
        if not isinstance(values, torch.Tensor):
            return self._upload(to_host(values).view(np.int32))
        _device_tensor(self.ctx.device, values, name, torch.int32, cols=cols)
        if cols is None and values.dim() != 1:
            raise ValueError(f"{name} must be an [S] tensor, not {tuple(values.shape)}")
        return values

    def _torch_dtype(self, dtype):
        import torch
        if np.dtype(dtype).names:
            return torch.int32
        return {"u": {4: torch.int32, 8: torch.int64}, "f": {4: torch.float32}}[
            np.dtype(dtype).kind][np.dtype(dtype).itemsize]

    def _shape(self, shape, dtype) -> tuple:
        return (tuple(shape) if isinstance(shape, tuple) else (shape,)) + _width(dtype)

    def alloc(self, shape, dtype):
        import torch
        return torch.empty(self._shape(shape, dtype), dtype=self._torch_dtype(dtype),
                           device=self.dev)

    def zeros(self, shape, dtype):
        import torch
        return torch.zeros(self._shape(shape, dtype), dtype=self._torch_dtype(dtype),
                           device=self.dev)

    def out(self, out, name: str, dtype, shape=None):
        """The caller's output tensor: of ``shape`` rows of ``dtype``, or (``shape`` None) any
        number of them."""
        if shape is not None:
            return _device_tensor(self.ctx.device, out, name, self._torch_dtype(dtype),
                                  shape=self._shape(shape, dtype))
        return _device_tensor(self.ctx.device, out, name, self._torch_dtype(dtype),
                              cols=_width(dtype)[0])

    def from_host(self, a, dtype=np.float32):
        return self._upload(np.ascontiguousarray(a, dtype=dtype))

    def uploads_done(self):
        import torch
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream())

    def keep(self, *owners):
        made, self._made = self._made, []
        if self.stream is not None:
            for t in (*made, *owners):
                if t is not None:
                    t.record_stream(self.stream)

    def finish(self):
        if self.stream is not None:
            self.stream.synchronize()

    def trim(self, buffer, count: int):
        return buffer

    def to_host(self, t, dtype, count=None):
        return tensor_to_host(t if count is None else t[:count], dtype)

    def isaf_operator(self, bits, words_per_sample: int, num_sites: int, fit):
        from .pcrelate import DeviceIsafOperator
        return DeviceIsafOperator(self.ctx, bits, words_per_sample, num_sites, fit)


HOST = HostPlace()
