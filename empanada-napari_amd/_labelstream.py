"""What the label tools (metrics.py, labels.py) share on the host: the sources a label array can come from, the double-buffered
slab stream over them, the sink a result goes to row by row, and the device table that grows when it is too small.  Nothing here
knows what a tool counts.

The stream keeps the staging buffers safe by itself: a slot is refilled only after everything the consumer queued on the slab it
held, so a consumer never synchronises the host for the stream's sake.  The staging buffers, their slots and the pinned download
buffer are this module's alone: a consumer sees device addresses, ``slab_bytes`` and a ``Sink``."""
import ctypes as C

import numpy as np
import torch

from . import _abi

SLAB_BYTES = 64 << 20      # default slab of a host array / chunked store: this many bytes of the wider side


def hp(a):
    return a.ctypes.data_as(C.c_void_p)


def initial_capacity(n):
    """First capacity (slots, a power of two) of the device table for ``n`` voxels: one slot per 64 voxels, at least 2^16
    (1 MiB) and at most 2^22 (64 MiB).  A label volume whose objects are more than a few voxels wide has far fewer
    distinct pairs than that; one that has more makes the table double (``LabelOverlap.doublings``)."""
    c = 1 << 16
    while c < (1 << 22) and c * 64 < n:
        c <<= 1
    return c


def need_device():
    if not torch.cuda.is_available():
        raise RuntimeError('empanada_napari_amd needs a HIP device (MI355X); there is no CPU fallback')
    _abi.load()


def pick_device(device, *arrays):
    if device is None:
        dev_in = [x.device for x in arrays if isinstance(x, torch.Tensor) and x.is_cuda]
        device = dev_in[0] if dev_in else torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


# ----------------------------------------------------------------------------
# sources: device tensors, host arrays, chunked stores
# ----------------------------------------------------------------------------
_EBYTES = {np.dtype(np.int8): -1, np.dtype(np.int16): -2, np.dtype(np.int32): -4, np.dtype(np.int64): -8,
           np.dtype(np.uint8): 1, np.dtype(np.uint16): 2, np.dtype(np.uint32): 4, np.dtype(np.uint64): 8, np.dtype(np.bool_): 1}


def ebytes(dtype):
    """element size as the kernels take it: 1, 2, 4 or 8, negative for a signed type"""
    try:
        return _EBYTES[np.dtype(str(dtype).replace('torch.', ''))]
    except (KeyError, TypeError):
        raise TypeError(f'label arrays: dtype {dtype} is not an integer label type') from None


class RawSource:
    """a contiguous device buffer with a given element size and shape (no dtype of torch's needed): slabs are views, nothing is
    copied, and there is nothing to reserve or to stage"""
    is_host = False

    def __init__(self, t, ebytes, shape):
        self.t = t
        self.ebytes = ebytes
        self.shape = tuple(int(s) for s in shape)
        self.rows = self.shape[0] if self.shape else 1
        self.row_elems = int(np.prod(self.shape[1:], dtype=np.int64)) if self.shape else 1
        self.row_bytes = self.row_elems * abs(ebytes)

    def address(self, z0, z1, slot, stream):
        return self.t.data_ptr() + z0 * self.row_bytes

    def slab_bytes(self, k, z0, z1):
        """slab k = rows [z0, z1) as the device bytes whose address the stream handed out"""
        return self.t.reshape(-1).view(torch.uint8)[z0 * self.row_bytes:z1 * self.row_bytes]


class DeviceSource(RawSource):
    """a tensor that is on the device already"""

    def __init__(self, t, device):
        if t.device != device:
            raise ValueError(f'label arrays: tensor on {t.device}, table on {device}')
        self.dtype = t.dtype
        super().__init__(t if t.is_contiguous() else t.contiguous(), ebytes(t.dtype), t.shape)


class HostSource(RawSource):
    """a numpy array or a chunked store (zstore.DirArray, a zarr array): slabs of whole leading-axis slices go through two
    pinned staging buffers and two device buffers; the upload of a slab is queued on a copy stream before the count of the
    previous one is waited for"""
    is_host = True

    def __init__(self, x, device):
        self.x = x
        self.dtype = np.dtype(x.dtype)
        self.device = device
        self.events = [None, None]
        super().__init__(None, ebytes(self.dtype), x.shape)

    def reserve(self, slab_rows, copy_stream):
        nbytes = max(1, slab_rows * self.row_bytes)
        self.pinned = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev = [torch.empty(nbytes, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.copy_stream = copy_stream

    def stage(self, z0, z1, slot):
        block = self.x[z0:z1] if self.shape else self.x
        block = np.ascontiguousarray(np.asarray(block), dtype=self.dtype).reshape(-1)
        nbytes = block.size * abs(self.ebytes)
        if self.events[slot] is not None:
            self.events[slot].synchronize()      # the slot's last upload has read the pinned buffer (long ago, in practice)
        self.pinned[slot][:nbytes].numpy()[:] = block.view(np.uint8)
        with torch.cuda.stream(self.copy_stream):
            self.dev[slot][:nbytes].copy_(self.pinned[slot][:nbytes], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        self.events[slot] = ev

    def address(self, z0, z1, slot, stream):
        stream.wait_event(self.events[slot])
        return self.dev[slot].data_ptr()

    def slab_bytes(self, k, z0, z1):
        return self.dev[k & 1][:(z1 - z0) * self.row_bytes]


def source(x, device):
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            return DeviceSource(x, device)
        x = x.numpy()
    if not (hasattr(x, 'shape') and hasattr(x, 'dtype') and hasattr(x, '__getitem__')):
        x = np.asarray(x)
    return HostSource(x, device)


# ----------------------------------------------------------------------------
# the slab stream
# ----------------------------------------------------------------------------
def slab_plan(rows, host_row_bytes, slab):
    """(slab, bounds): how ``rows`` leading-axis entries are cut into slabs.  ``host_row_bytes``: the largest ``row_bytes`` of
    the sources that are on the host, None without one.  ``slab=None`` takes everything at once when nothing has to be
    uploaded, and about SLAB_BYTES of the widest host source otherwise.  A plan made from its own slab is the same plan, so a
    consumer that needs the size before the first slab plans first and hands the slab on."""
    if slab is None:
        slab = rows if host_row_bytes is None else max(1, SLAB_BYTES // max(1, host_row_bytes))
    slab = max(1, min(int(slab), max(rows, 1)))
    return slab, [(z, min(rows, z + slab)) for z in range(0, rows, slab)]


def stream_slabs(sources, slab, device):
    """Yields ``(k, z0, z1, [address per source])`` for every slab of ``slab_plan``, the addresses valid on the device's
    current stream.  Host sources are double-buffered: slab k + 1 is read, copied into its pinned buffer and queued on a copy
    stream before slab k is handed out, so that the upload runs under whatever the consumer launches on slab k.

    The guarantee: slab k stays as it was handed out until everything the consumer queued on that stream before it asked for
    slab k + 1 has run.  An event recorded then stands for that work, and the copy stream waits for it before it refills the slot
    (k & 1) with slab k + 2: the consumer need not synchronise the host, and the host does not stall for it."""
    rows = sources[0].rows
    host = [s for s in sources if s.is_host]
    slab, bounds = slab_plan(rows, max(s.row_bytes for s in host) if host else None, slab)
    stream = torch.cuda.current_stream(device)
    if host:
        copy_stream = torch.cuda.Stream(device=device)
        for s in host:
            s.reserve(slab, copy_stream)
    consumed = [None, None]      # per slot: the consumer's work on the slab it held last

    def stage(k):
        if k < len(bounds):
            if consumed[k & 1] is not None:
                copy_stream.wait_event(consumed[k & 1])
            for s in host:
                s.stage(*bounds[k], k & 1)
    stage(0)
    for k, (z0, z1) in enumerate(bounds):
        stage(k + 1)
        yield k, z0, z1, [s.address(z0, z1, k & 1, stream) for s in sources]
        if host:
            consumed[k & 1] = stream.record_event()


# ----------------------------------------------------------------------------
# the sink
# ----------------------------------------------------------------------------
class Sink:
    """Where a result of ``shape`` and ``dtype`` goes, rows [z0, z1) of the leading axis at a time.  ``dest``: a contiguous device
    tensor, which a kernel writes through ``address``; or a numpy array or a chunked store (anything with ``__setitem__``), which
    gets the rows a kernel left on the device through ``write``.  ``dest=None`` is a new array, made when it is first needed: a
    tensor on ``device``, a numpy array without one."""

    def __init__(self, dest, shape, dtype, device=None):
        self.dest, self.shape, self.device = dest, tuple(int(s) for s in shape), device
        self.dtype = dtype if isinstance(dtype, torch.dtype) else np.dtype(dtype)
        self.is_host = device is None if dest is None else not isinstance(dest, torch.Tensor)
        self.row_bytes = int(np.prod(self.shape[1:], dtype=np.int64)) * abs(ebytes(self.dtype))
        self.back = None

    def made(self):
        if self.dest is None:
            self.dest = np.empty(self.shape, self.dtype) if self.is_host else torch.empty(self.shape, dtype=self.dtype, device=self.device)
        return self.dest

    def address(self, z0):
        """device destination: where its row z0 begins"""
        return self.made().data_ptr() + z0 * self.row_bytes

    def put(self, z0, z1, host):
        """host destination: rows [z0, z1), on the host as the bytes ``host``, are written.  The whole of a new array is that array."""
        arr = host.numpy().view(self.dtype).reshape((z1 - z0,) + self.shape[1:])
        if self.dest is None and (z0, z1) == (0, self.shape[0]):
            self.dest = arr
        else:
            self.made()[z0:z1] = arr
        return self.dest

    def write(self, z0, z1, dev_bytes):
        """host destination: rows [z0, z1) lie at the head of the device bytes ``dev_bytes``.  They come down through a pinned buffer
        as large as the first, the largest, slab: the one place where the label tools synchronise for a download"""
        self.made()
        nbytes = (z1 - z0) * self.row_bytes
        if self.back is None:
            self.back = torch.empty(max(1, nbytes), dtype=torch.uint8).pin_memory()
        self.back[:nbytes].copy_(dev_bytes[:nbytes], non_blocking=True)
        torch.cuda.current_stream(dev_bytes.device).synchronize()
        self.put(z0, z1, self.back[:nbytes])


# ----------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------
class GrowableTable:
    """The open-addressing table of one kernel family on the device, behind the family's five C entries ``<prefix>_work_bytes,
    _reset, _accumulate, _grow, _finalize``.  ``what`` names the tool in the capacity error."""

    def __init__(self, prefix, what, capacity, device):
        self.lib = _abi.load()
        self.prefix = prefix
        self.what = what
        self.device = device
        self.doublings = 0
        self.capacity = int(capacity)
        self.buf = self._new(self.capacity)

    def _call(self, entry, *args):
        name = f'{self.prefix}_{entry}'
        _abi.check(getattr(self.lib, name)(*args), name)

    def _new(self, capacity):
        nbytes = getattr(self.lib, f'{self.prefix}_work_bytes')(capacity)
        if nbytes == 0:
            raise ValueError(f'{self.what}: capacity {capacity} is not a power of two in [64, 2^32]')
        buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._call('reset', _abi.ptr(buf), capacity, _abi.stream_ptr(self.device))
        return buf

    def _grow(self):
        cap = self.capacity
        while True:
            cap *= 2
            new = self._new(cap)
            ov = C.c_int(0)
            self._call('grow', _abi.ptr(self.buf), self.capacity, _abi.ptr(new), cap, _abi.stream_ptr(self.device), C.byref(ov))
            self.doublings += 1
            if not ov.value:
                break
        self.buf, self.capacity = new, cap

    def add(self, *args):
        """one ``accumulate`` of the family: ``args`` are what it takes in front of (table, capacity, stream, &overflow).  Returns
        with the stream synchronised and the slab counted, after growing the table as often as that takes."""
        while True:
            ov = C.c_int(0)
            self._call('accumulate', *args, _abi.ptr(self.buf), self.capacity, _abi.stream_ptr(self.device), C.byref(ov))
            if not ov.value:
                return
            self._grow()      # the failed call has taken its own additions out again: count the slab once more

    def finalize(self, extra=()):
        """(keys, counts, *extras) on the device, sorted by key.  ``extra``: (columns, dtype) of every further per-row output
        the family's finalize writes, between counts and max_out."""
        num = C.c_int64(0)      # first call: the number of rows only, so that the buffers are as long as the result
        stream = _abi.stream_ptr(self.device)
        self._call('finalize', _abi.ptr(self.buf), self.capacity, None, None, *(None for _ in extra), 0, C.byref(num), stream)
        k = num.value
        out = [torch.empty(max(k, 1), dtype=torch.int64, device=self.device) for _ in range(2)]
        out += [torch.empty((max(k, 1), cols), dtype=dtype, device=self.device) for cols, dtype in extra]
        self._call('finalize', _abi.ptr(self.buf), self.capacity, *(_abi.ptr(t) for t in out), k, C.byref(num), stream)
        # the keys are unsigned: flip the sign bit so that the signed sort orders them
        flip = torch.iinfo(torch.int64).min
        skeys, order = torch.sort(out[0][:k] ^ flip)
        return (skeys ^ flip, *(t[:k][order] for t in out[1:]))
