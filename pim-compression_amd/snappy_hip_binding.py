"""ctypes binding of libsnappy_hip.so (include/snappy_hip.h) for the tests, bench.py and smoke().

Plumbing only: torch provides device memory and streams, every byte of codec work happens in
the HIP library.  There is no fallback: if the library or a GPU is missing, calls raise.
"""
import ctypes
import os

import numpy as np

# The drop-in pair's overlapped pipeline keeps six HIP streams busy; HIP maps streams onto GPU_MAX_HW_QUEUES hardware
# queues (default 4).  The host program owns its environment (the library never calls setenv), so this host-side module
# asks for 8 unless the variable is set already; it takes effect if HIP has not been initialised yet.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsnappy_hip.so")

SNAPPY_OK, SNAPPY_INVALID_INPUT, SNAPPY_BUFFER_TOO_SMALL = 0, 1, 2


class HostBufferContext(ctypes.Structure):
    """struct host_buffer_context, reference snappy/dpu_snappy.h:37-44."""
    _fields_ = [("file_name", ctypes.c_char_p), ("buffer", ctypes.c_void_p), ("curr", ctypes.c_void_p),
                ("length", ctypes.c_ulong), ("max", ctypes.c_ulong)]


class ProgramRuntime(ctypes.Structure):
    """struct program_runtime, reference snappy/dpu_snappy.h:47-55."""
    _fields_ = [(k, ctypes.c_double) for k in ("pre", "d_alloc", "load", "copy_in", "run", "copy_out", "d_free")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class StreamDesc(ctypes.Structure):
    """snappy_hip_stream_desc."""
    _fields_ = [("stream", ctypes.c_void_p), ("stream_len", ctypes.c_uint64), ("block_offsets", ctypes.c_void_p),
                ("result", ctypes.c_void_p), ("total_len", ctypes.c_uint32), ("block_size", ctypes.c_uint32),
                ("header_len", ctypes.c_uint32), ("num_blocks", ctypes.c_uint32)]


STREAM_DESC_DTYPE = np.dtype([("stream", "<u8"), ("stream_len", "<u8"), ("block_offsets", "<u8"), ("result", "<u8"),
                              ("total_len", "<u4"), ("block_size", "<u4"), ("header_len", "<u4"), ("num_blocks", "<u4")])

_LIB = None
_LIBC = None


class CheckReport(ctypes.Structure):            # snappy_hip_check_report
    _fields_ = [("blocks", ctypes.c_uint64), ("bad_blocks", ctypes.c_uint64), ("first_bad_block", ctypes.c_uint64),
                ("first_bad_offset", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SnappyHipError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise SnappyHipError(f"{LIB_PATH} is missing: build it (python -c 'import __graft_entry__ as g; g.build()')")
        L = ctypes.CDLL(LIB_PATH)
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.snappy_hip_device_count.restype = ctypes.c_int
        L.snappy_hip_set_device.restype = ctypes.c_int
        L.snappy_hip_set_device.argtypes = [ctypes.c_int]
        L.snappy_hip_last_error.restype = ctypes.c_char_p
        L.snappy_hip_arch.restype = ctypes.c_char_p
        L.snappy_hip_slot_stride.restype = u32
        L.snappy_hip_slot_stride.argtypes = [u32]
        L.snappy_hip_num_blocks.restype = u64
        L.snappy_hip_num_blocks.argtypes = [u64, u32]
        L.snappy_hip_stream_bound.restype = u64
        L.snappy_hip_stream_bound.argtypes = [u64, u32]
        L.snappy_hip_write_header.restype = u32
        L.snappy_hip_write_header.argtypes = [vp, u32, u32]
        L.snappy_hip_parse_header.restype = u32
        L.snappy_hip_parse_header.argtypes = [vp, u64, ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.snappy_hip_compress_blocks.restype = ctypes.c_int
        L.snappy_hip_compress_blocks.argtypes = [vp, u64, u32, vp, u32, vp, vp, u64, vp]
        L.snappy_hip_compress_blocks_batch.restype = ctypes.c_int
        L.snappy_hip_compress_blocks_batch.argtypes = [vp, u32, u32, u32, vp, u64, vp]
        L.snappy_hip_compress_scratch_bytes.restype = u64
        L.snappy_hip_k1_lds_waves_per_cu.restype = u32
        L.snappy_hip_k1_lds_waves_per_cu.argtypes = [u32]
        L.snappy_hip_compact.restype = ctypes.c_int
        L.snappy_hip_compact.argtypes = [vp, u32, vp, u64, u32, vp, vp, vp, vp]
        L.snappy_hip_index_streams.restype = ctypes.c_int
        L.snappy_hip_index_streams.argtypes = [vp, u32, vp]
        L.snappy_hip_decompress_blocks_batch.restype = ctypes.c_int
        L.snappy_hip_decompress_blocks_batch.argtypes = [vp, u32, u32, vp]
        L.snappy_hip_verify_index.restype = ctypes.c_int
        L.snappy_hip_verify_index.argtypes = [vp, u32, vp]
        L.snappy_hip_decompress_blocks.restype = ctypes.c_int
        L.snappy_hip_decompress_blocks.argtypes = [vp, u64, vp, u64, u32, vp, vp, vp]
        L.snappy_hip_decompress_blocks_wide.restype = ctypes.c_int
        L.snappy_hip_decompress_blocks_wide.argtypes = [vp, u64, vp, u64, u32, vp, vp, u32, vp, vp]
        L.snappy_decompress_wide_gpu.restype = ctypes.c_int
        L.snappy_decompress_wide_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u32,
                                                 ctypes.POINTER(ProgramRuntime)]
        L.snappy_hip_decompress_ranges_scratch_bytes.restype = u64
        L.snappy_hip_decompress_ranges_scratch_bytes.argtypes = [u32, u32]
        L.snappy_hip_decompress_ranges.restype = ctypes.c_int
        L.snappy_hip_decompress_ranges.argtypes = [vp, u32, vp, u32, vp, u32, vp, u64, vp]
        L.snappy_decompress_range_gpu.restype = ctypes.c_int
        L.snappy_decompress_range_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u64, u64,
                                                  ctypes.POINTER(ProgramRuntime)]
        L.snappy_hip_update_scratch_bytes.restype = u64
        L.snappy_hip_update_scratch_bytes.argtypes = [u32, u32, u32, u32]
        L.snappy_hip_update_ranges.restype = ctypes.c_int
        L.snappy_hip_update_ranges.argtypes = [vp, u32, u32, vp, u32, vp, vp, u64, vp, vp, vp, u32, vp, u64, vp]
        L.snappy_hip_resize_scratch_bytes.restype = u64
        L.snappy_hip_resize_scratch_bytes.argtypes = [u32, u32, u32, u32, u32]
        L.snappy_hip_resize.restype = ctypes.c_int
        L.snappy_hip_resize.argtypes = [vp, u32, u32, u32, u32, vp, u32, vp, vp, u64, vp, vp, vp, vp, u64, vp]
        L.snappy_resize_gpu.restype = ctypes.c_int
        L.snappy_resize_gpu.argtypes = [ctypes.POINTER(HostBufferContext), u64, ctypes.POINTER(HostBufferContext),
                                        ctypes.POINTER(HostBufferContext), ctypes.POINTER(ProgramRuntime)]
        L.snappy_hip_raw_decompress_batch.restype = ctypes.c_int
        L.snappy_hip_raw_decompress_batch.argtypes = [vp, u32, vp, vp, vp]
        L.snappy_hip_raw_decompress_split_scratch_bytes.restype = u64
        L.snappy_hip_raw_decompress_split_scratch_bytes.argtypes = [u32, u32, u32, u64, u64]
        L.snappy_hip_raw_decompress_split_batch.restype = ctypes.c_int
        L.snappy_hip_raw_decompress_split_batch.argtypes = [vp, u32, u32, u32, u64, u64, vp, vp, vp, vp, u64, vp]
        L.snappy_decompress_raw_split_gpu.restype = ctypes.c_int
        L.snappy_decompress_raw_split_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u32,
                                                      ctypes.POINTER(ProgramRuntime)]
        L.snappy_hip_raw_compress_bound.restype = u64
        L.snappy_hip_raw_compress_bound.argtypes = [u64, u32]
        L.snappy_hip_raw_compress_scratch_bytes.restype = u64
        L.snappy_hip_raw_compress_scratch_bytes.argtypes = [u32, u32, u32]
        L.snappy_hip_raw_compress_batch.restype = ctypes.c_int
        L.snappy_hip_raw_compress_batch.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, u64, vp]
        L.snappy_hip_raw_compress_batch_tables.restype = ctypes.c_int
        L.snappy_hip_raw_compress_batch_tables.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, u64, vp, u64, vp]
        L.snappy_hip_sz_compress_batch_tables.restype = ctypes.c_int
        L.snappy_hip_sz_compress_batch_tables.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, u64, vp, u64, vp]
        L.snappy_compress_raw_tables_gpu.restype = ctypes.c_int
        L.snappy_compress_raw_tables_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u32,
                                                     ctypes.POINTER(ProgramRuntime)]
        L.snappy_compress_sz_tables_gpu.restype = ctypes.c_int
        L.snappy_compress_sz_tables_gpu.argtypes = L.snappy_compress_raw_tables_gpu.argtypes
        L.snappy_hip_crc32c_batch.restype = ctypes.c_int
        L.snappy_hip_crc32c_batch.argtypes = [vp, u32, vp, vp]
        L.snappy_hip_sz_decompress_scratch_bytes.restype = u64
        L.snappy_hip_sz_decompress_scratch_bytes.argtypes = [u32, u32]
        L.snappy_hip_sz_decompress_batch.restype = ctypes.c_int
        L.snappy_hip_sz_decompress_batch.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, vp, u64, vp]
        L.snappy_hip_sz_decompress_split_scratch_bytes.restype = u64
        L.snappy_hip_sz_decompress_split_scratch_bytes.argtypes = [u32, u32, u32, u64]
        L.snappy_hip_sz_decompress_split_batch.restype = ctypes.c_int
        L.snappy_hip_sz_decompress_split_batch.argtypes = [vp, u32, u32, u32, u64, u32, vp, vp, vp, vp, vp, u64, vp]
        L.snappy_hip_sz_index_scratch_bytes.restype = u64
        L.snappy_hip_sz_index_scratch_bytes.argtypes = [u32, u32, u32, u64]
        L.snappy_hip_sz_index_batch.restype = ctypes.c_int
        L.snappy_hip_sz_index_batch.argtypes = [vp, u32, u32, u32, u64, vp, vp, vp, vp, vp, u64, vp]
        L.snappy_hip_sz_decompress_ranges_scratch_bytes.restype = u64
        L.snappy_hip_sz_decompress_ranges_scratch_bytes.argtypes = [u32]
        L.snappy_hip_sz_decompress_ranges.restype = ctypes.c_int
        L.snappy_hip_sz_decompress_ranges.argtypes = [vp, u32, vp, u32, u32, vp, vp, vp, u64, vp]
        L.snappy_hip_sz_compress_bound.restype = u64
        L.snappy_hip_sz_compress_bound.argtypes = [u64, u32]
        L.snappy_hip_sz_compress_scratch_bytes.restype = u64
        L.snappy_hip_sz_compress_scratch_bytes.argtypes = [u32, u32, u32]
        L.snappy_hip_sz_compress_batch.restype = ctypes.c_int
        L.snappy_hip_sz_compress_batch.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, u64, vp]
        L.snappy_compress_sz_gpu.restype = ctypes.c_int
        L.snappy_compress_sz_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u32,
                                             ctypes.POINTER(ProgramRuntime)]
        L.snappy_decompress_sz_gpu.restype = ctypes.c_int
        L.snappy_decompress_sz_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u32,
                                               ctypes.POINTER(ProgramRuntime)]
        L.snappy_decompress_sz_range_gpu.restype = ctypes.c_int
        L.snappy_decompress_sz_range_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u64, u64, u32,
                                                     ctypes.POINTER(ProgramRuntime)]
        L.snappy_decompress_sz_split_gpu.restype = ctypes.c_int
        L.snappy_decompress_sz_split_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u32,
                                                     ctypes.POINTER(ProgramRuntime)]
        L.snappy_hip_check_scratch_bytes.restype = u64
        L.snappy_hip_check_scratch_bytes.argtypes = [u32]
        L.snappy_hip_check_blocks.restype = ctypes.c_int
        L.snappy_hip_check_blocks.argtypes = [vp, u32, vp, vp, vp, u64, vp]
        L.snappy_hip_raw_check_batch.restype = ctypes.c_int
        L.snappy_hip_raw_check_batch.argtypes = [vp, u32, vp, vp, vp]
        L.snappy_hip_raw_check_split_scratch_bytes.restype = u64
        L.snappy_hip_raw_check_split_scratch_bytes.argtypes = [u32, u32, u64]
        L.snappy_hip_raw_check_split_batch.restype = ctypes.c_int
        L.snappy_hip_raw_check_split_batch.argtypes = [vp, u32, u32, u64, vp, vp, vp, vp, u64, vp]
        L.snappy_check_gpu.restype = ctypes.c_int
        L.snappy_check_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(CheckReport), ctypes.POINTER(ProgramRuntime)]
        L.snappy_check_raw_gpu.restype = ctypes.c_int
        L.snappy_check_raw_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(u64), ctypes.POINTER(ProgramRuntime)]
        L.snappy_check_raw_split_gpu.restype = ctypes.c_int
        L.snappy_check_raw_split_gpu.argtypes = L.snappy_check_raw_gpu.argtypes
        L.snappy_update_range_gpu.restype = ctypes.c_int
        L.snappy_update_range_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u64,
                                              ctypes.POINTER(HostBufferContext), ctypes.POINTER(ProgramRuntime)]
        L.snappy_compress_raw_gpu.restype = ctypes.c_int
        L.snappy_compress_raw_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u32,
                                              ctypes.POINTER(ProgramRuntime)]
        L.snappy_decompress_raw_gpu.restype = ctypes.c_int
        L.snappy_decompress_raw_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext),
                                                ctypes.POINTER(ProgramRuntime)]
        L.snappy_compress_gpu.restype = ctypes.c_int
        L.snappy_compress_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext), u32,
                                          ctypes.POINTER(ProgramRuntime)]
        L.snappy_decompress_gpu.restype = ctypes.c_int
        L.snappy_decompress_gpu.argtypes = [ctypes.POINTER(HostBufferContext), ctypes.POINTER(HostBufferContext),
                                            ctypes.POINTER(ProgramRuntime)]
        _LIB = L
    return _LIB


def libc():
    global _LIBC
    if _LIBC is None:
        _LIBC = ctypes.CDLL(None)
        _LIBC.free.argtypes = [ctypes.c_void_p]
        _LIBC.malloc.restype = ctypes.c_void_p
        _LIBC.malloc.argtypes = [ctypes.c_size_t]
    return _LIBC


def _check(rc, what):
    if rc != 0:
        raise SnappyHipError(f"{what} failed ({rc}): {lib().snappy_hip_last_error().decode()}")


def slot_stride(block_size):
    return int(lib().snappy_hip_slot_stride(block_size))


def num_blocks(n, block_size):
    return int(lib().snappy_hip_num_blocks(n, block_size))


def shard_block_range(num_blocks_total, shards, shard):
    """(first_block, block_count) of `shard` when a file of `num_blocks_total` blocks is split over `shards` devices: the
    contiguous ranges of ceil(B / G) blocks that snappy_compress_gpu / snappy_decompress_gpu use (csrc/dropin_plan.hpp),
    i.e. the partitioning of the reference's input_blocks_per_dpu (snappy_compress.c:494-520)."""
    per = (num_blocks_total + shards - 1) // shards if num_blocks_total else 0
    first = min(num_blocks_total, shard * per)
    return first, min(num_blocks_total, first + per) - first


def k1_lds_waves_per_cu(block_size):
    return int(lib().snappy_hip_k1_lds_waves_per_cu(block_size))


def write_header(total_len, block_size):
    buf = (ctypes.c_uint8 * 10)()
    k = lib().snappy_hip_write_header(buf, total_len, block_size)
    return bytes(buf[:k])


def parse_header(data):
    a = np.frombuffer(data[:10], dtype=np.uint8).copy()
    total, bs = ctypes.c_uint32(), ctypes.c_uint32()
    h = lib().snappy_hip_parse_header(a.ctypes.data, a.size, ctypes.byref(total), ctypes.byref(bs))
    if h == 0:
        raise ValueError("malformed header")
    return total.value, bs.value, h


# ---------------------------------------------------------------------------
# resident API (device tensors)
# ---------------------------------------------------------------------------

def _stream_handle(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class CompressWorkspace:
    """Device buffers for compressing containers of up to `max_len` bytes at `block_size`."""

    def __init__(self, max_len, block_size, device="cuda", scratch=True):
        """scratch=False: no hash-table workspace of its own (a batch launch uses one workspace's scratch for all)."""
        import torch
        self._torch = torch
        self.block_size = block_size
        self.max_len = max_len
        self.stride = slot_stride(block_size)
        nb = num_blocks(max_len, block_size)
        self.slots = torch.empty(max(nb, 1) * self.stride, dtype=torch.uint8, device=device)
        self.block_bytes = torch.empty(max(nb, 1), dtype=torch.int32, device=device)
        self.offsets = torch.empty(nb + 1, dtype=torch.int64, device=device)
        self.stream_len = torch.zeros(1, dtype=torch.int64, device=device)
        self.scratch_bytes = int(lib().snappy_hip_compress_scratch_bytes()) if scratch else 0
        self.scratch = torch.empty(self.scratch_bytes + 256, dtype=torch.uint8, device=device) if scratch else None
        self.scratch_ptr = ((self.scratch.data_ptr() + 255) & ~255) if scratch else 0

    def lds_form_blocks(self):
        """Blocks of the last compress_blocks() launch that were taken by the LDS-table wavefronts (statistics)."""
        off = self.scratch_ptr - self.scratch.data_ptr()
        return int(self.scratch[off + 16:off + 20].view(self._torch.int32).item())

    def stream_capacity(self, n):
        return int(lib().snappy_hip_stream_bound(n, self.block_size))


def compress_blocks(d_in, n, ws):
    """K1 only: per-block compress into ws.slots / ws.block_bytes (async on the current stream)."""
    import torch
    _check(lib().snappy_hip_compress_blocks(d_in.data_ptr(), n, ws.block_size, ws.slots.data_ptr(), ws.stride,
                                            ws.block_bytes.data_ptr(), ws.scratch_ptr, ws.scratch_bytes,
                                            _stream_handle(torch)), "snappy_hip_compress_blocks")


class _CompressItem(ctypes.Structure):          # struct snappy_hip_compress_item
    _fields_ = [("d_input", ctypes.c_void_p), ("input_len", ctypes.c_uint64), ("d_slots", ctypes.c_void_p),
                ("d_block_bytes", ctypes.c_void_p)]


def compress_blocks_batch(jobs, scratch_ws=None):
    """K1 over several containers in one launch.  jobs: list of (d_in, n, ws); every ws has its own slots / block_bytes,
    the scratch of `scratch_ws` (default: the first job's) is the launch's hash-table workspace."""
    import torch
    if not jobs:
        return
    sw = scratch_ws or jobs[0][2]
    items = (_CompressItem * len(jobs))()
    for k, (d_in, n, ws) in enumerate(jobs):
        assert ws.block_size == sw.block_size and ws.stride == sw.stride
        items[k] = _CompressItem(d_in.data_ptr(), n, ws.slots.data_ptr(), ws.block_bytes.data_ptr())
    _check(lib().snappy_hip_compress_blocks_batch(ctypes.cast(items, ctypes.c_void_p), len(jobs), sw.block_size, sw.stride,
                                                  sw.scratch_ptr, sw.scratch_bytes, _stream_handle(torch)),
           "snappy_hip_compress_blocks_batch")


def compact(n, ws, d_stream):
    """scan + gather into d_stream (async); ws.stream_len[0] holds the stream length afterwards."""
    import torch
    _check(lib().snappy_hip_compact(ws.slots.data_ptr(), ws.stride, ws.block_bytes.data_ptr(), n, ws.block_size,
                                    d_stream.data_ptr(), ws.offsets.data_ptr(), ws.stream_len.data_ptr(),
                                    _stream_handle(torch)), "snappy_hip_compact")


def compress_resident(d_in, block_size=32768, n=None):
    """Compress a uint8 CUDA tensor; returns the framed stream as a CUDA uint8 tensor (exact length)."""
    import torch
    n = d_in.numel() if n is None else n
    ws = CompressWorkspace(n, block_size, d_in.device)
    d_stream = torch.empty(ws.stream_capacity(n) + 16, dtype=torch.uint8, device=d_in.device)
    compress_blocks(d_in, n, ws)
    compact(n, ws, d_stream)
    length = int(ws.stream_len.item())
    return d_stream[:length]


def make_stream_descs(entries, device="cuda"):
    """entries: list of dicts(stream=tensor, stream_len, block_offsets=tensor, result=tensor, total_len, block_size,
    header_len, num_blocks) -> device tensor of packed snappy_hip_stream_desc."""
    import torch
    arr = np.zeros(len(entries), dtype=STREAM_DESC_DTYPE)
    for i, e in enumerate(entries):
        arr[i] = (e["stream"].data_ptr(), e["stream_len"], e["block_offsets"].data_ptr(), e["result"].data_ptr(),
                  e["total_len"], e["block_size"], e["header_len"], e["num_blocks"])
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


def index_streams(d_descs, count):
    import torch
    _check(lib().snappy_hip_index_streams(d_descs.data_ptr(), count, _stream_handle(torch)), "snappy_hip_index_streams")


def verify_index(d_descs, count):
    """Parallel check of candidate indexes (num_blocks + 1 offsets per stream) against the streams' size chains."""
    import torch
    _check(lib().snappy_hip_verify_index(d_descs.data_ptr(), count, _stream_handle(torch)), "snappy_hip_verify_index")


def decompress_blocks(d_stream, stream_len, d_block_offsets, total_len, block_size, d_out, d_status):
    import torch
    _check(lib().snappy_hip_decompress_blocks(d_stream.data_ptr(), stream_len, d_block_offsets.data_ptr(), total_len,
                                              block_size, d_out.data_ptr(), d_status.data_ptr(), _stream_handle(torch)),
           "snappy_hip_decompress_blocks")


WIDE_MAX_BLOCK, WIDE_MAX_CSZ = 32768, 38400      # SNAPPY_HIP_WIDE_MAX_BLOCK, SNAPPY_HIP_WIDE_MAX_CSZ


def decompress_blocks_wide(d_stream, stream_len, d_block_offsets, total_len, block_size, d_out, d_status, d_result, waves_per_block=0):
    """snappy_hip_decompress_blocks_wide: K2's arguments and answers, a workgroup of waves_per_block wavefronts (0 = 16) on every
    block.  d_result: 4 int32 on the device (blocks decoded wide, sent to the serial decoder by the limits, not proven, 0)."""
    import torch
    _check(lib().snappy_hip_decompress_blocks_wide(d_stream.data_ptr() if d_stream is not None else None, stream_len,
                                                   d_block_offsets.data_ptr() if d_block_offsets is not None else None, total_len, block_size,
                                                   d_out.data_ptr() if d_out is not None else None,
                                                   d_status.data_ptr() if d_status is not None else None, waves_per_block,
                                                   d_result.data_ptr() if d_result is not None else None, _stream_handle(torch)),
           "snappy_hip_decompress_blocks_wide")


class _DecompressItem(ctypes.Structure):        # struct snappy_hip_decompress_item
    _fields_ = [("d_stream", ctypes.c_void_p), ("stream_len", ctypes.c_uint64), ("d_stream_len", ctypes.c_void_p),
                ("d_block_offsets", ctypes.c_void_p), ("total_len", ctypes.c_uint64), ("d_out", ctypes.c_void_p),
                ("d_status", ctypes.c_void_p)]


def decompress_blocks_batch(jobs, block_size):
    """K2 over several streams in one launch.  jobs: list of (d_stream, stream_len, d_block_offsets, total_len, d_out, d_status);
    stream_len is an int, or a device int64 tensor of one element (the length stays on the device)."""
    import torch
    if not jobs:
        return
    items = (_DecompressItem * len(jobs))()
    for k, (d_stream, slen, d_off, total, d_out, d_status) in enumerate(jobs):
        on_dev = hasattr(slen, "data_ptr")
        items[k] = _DecompressItem(d_stream.data_ptr(), 0 if on_dev else slen, slen.data_ptr() if on_dev else None, d_off.data_ptr(),
                                   total, d_out.data_ptr(), d_status.data_ptr())
    _check(lib().snappy_hip_decompress_blocks_batch(ctypes.cast(items, ctypes.c_void_p), len(jobs), block_size,
                                                    _stream_handle(torch)), "snappy_hip_decompress_blocks_batch")


def decompress_resident(d_stream, stream_len=None):
    """Decode a framed stream held in a CUDA uint8 tensor; returns (status, plaintext CUDA tensor)."""
    import torch
    stream_len = d_stream.numel() if stream_len is None else stream_len
    head = bytes(d_stream[:min(10, stream_len)].cpu().numpy())
    total, bs, hdr = parse_header(head)
    nb = num_blocks(total, bs) if bs else 0
    dev = d_stream.device
    d_out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    if nb == 0:
        return (0 if stream_len == hdr else 1), d_out[:total]
    d_boff = torch.empty(nb, dtype=torch.int64, device=dev)
    d_res = torch.full((2,), 7, dtype=torch.int32, device=dev)
    d_status = torch.full((nb,), 9, dtype=torch.int32, device=dev)
    descs = make_stream_descs([dict(stream=d_stream, stream_len=stream_len, block_offsets=d_boff, result=d_res,
                                    total_len=total, block_size=bs, header_len=hdr, num_blocks=nb)], dev)
    index_streams(descs, 1)
    res = d_res.cpu().numpy()
    if res[0] != 0 or res[1] != nb:
        return 1, d_out[:total]
    decompress_blocks(d_stream, stream_len, d_boff, total, bs, d_out, d_status)
    bad = int((d_status != 0).sum().item())
    return (1 if bad else 0), d_out[:total]


# byte ranges of framed containers (snappy_hip_decompress_ranges)
RANGE_OUT_OF_BOUNDS = 2
RANGE_DTYPE = np.dtype([("offset", "<u8"), ("length", "<u8"), ("dst", "<u8"), ("stream", "<u4"), ("pad", "<u4")])   # snappy_hip_range


def decompress_ranges_scratch_bytes(max_block_size, range_count):
    """Scratch for a full grid of snappy_hip_decompress_ranges on the current device (0 for a bad max_block_size)."""
    return int(lib().snappy_hip_decompress_ranges_scratch_bytes(max_block_size, range_count))


def make_ranges(entries, device="cuda"):
    """entries: list of (stream index, offset, length, dst) with dst a device address (int) -> device tensor of snappy_hip_range."""
    import torch
    arr = np.zeros(len(entries), dtype=RANGE_DTYPE)
    for i, (s, off, length, dst) in enumerate(entries):
        arr[i] = (off, length, dst, s, 0)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


def decompress_ranges(d_descs, count, d_ranges, range_count, d_status, max_block_size, d_scratch=None):
    """Enqueue snappy_hip_decompress_ranges on the current stream.  d_descs: make_stream_descs() tensor (block_offsets filled
    in), d_ranges: make_ranges() tensor or any device uint8 tensor of packed snappy_hip_range, d_status: device int32 tensor of
    range_count entries.  d_scratch: 256-byte aligned device uint8 tensor (default: a fresh one for the full grid)."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(decompress_ranges_scratch_bytes(max_block_size, range_count), dtype=torch.uint8, device=d_status.device)
    _check(lib().snappy_hip_decompress_ranges(d_descs.data_ptr(), count, d_ranges.data_ptr(), range_count, d_status.data_ptr(),
                                              max_block_size, d_scratch.data_ptr(), d_scratch.numel(), _stream_handle(torch)),
           "snappy_hip_decompress_ranges")
    return d_scratch


# overwriting byte ranges of one container (snappy_hip_update_ranges)
WRITE_UNORDERED = 3
UPDATE_REJECTED = 4
WRITE_DTYPE = np.dtype([("offset", "<u8"), ("length", "<u8"), ("src", "<u8"), ("pad", "<u8")])   # snappy_hip_write


def update_scratch_bytes(block_size, blocks, write_count, max_dirty_blocks):
    """Scratch of snappy_hip_update_ranges on the current device (0 for a bad block size)."""
    return int(lib().snappy_hip_update_scratch_bytes(block_size, blocks, write_count, max_dirty_blocks))


def make_writes(entries, device="cuda"):
    """entries: list of (offset, length, src) with src a device address (int), sorted by offset and disjoint -> device tensor
    of snappy_hip_write."""
    import torch
    arr = np.zeros(max(len(entries), 1), dtype=WRITE_DTYPE)
    for i, (off, length, src) in enumerate(entries):
        arr[i] = (off, length, src, 0)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


def update_ranges(d_desc, total_len, block_size, d_writes, write_count, d_write_status, d_new_stream, d_new_offsets, d_new_stream_len,
                  d_result, max_dirty_blocks, d_scratch=None, capacity=None):
    """Enqueue snappy_hip_update_ranges on the current stream.  d_desc: make_stream_descs() tensor of ONE descriptor
    (block_offsets filled in), d_writes: make_writes() tensor, d_write_status: device int32 tensor of write_count entries,
    d_new_stream: device uint8 tensor (capacity: its size), d_new_offsets: device int64 tensor of num_blocks + 1 entries,
    d_new_stream_len: device int64 tensor of one entry, d_result: device int32 tensor of two.  d_scratch: 256-byte aligned
    device uint8 tensor (default: a fresh one).  Nothing is synchronised."""
    import torch
    nb = num_blocks(total_len, block_size)
    if d_scratch is None:
        d_scratch = torch.empty(update_scratch_bytes(block_size, nb, write_count, max_dirty_blocks), dtype=torch.uint8, device=d_new_stream.device)
    _check(lib().snappy_hip_update_ranges(d_desc.data_ptr(), total_len, block_size, d_writes.data_ptr() if write_count else None, write_count,
                                          d_write_status.data_ptr() if write_count else None, d_new_stream.data_ptr(),
                                          d_new_stream.numel() if capacity is None else capacity, d_new_offsets.data_ptr(),
                                          d_new_stream_len.data_ptr(), d_result.data_ptr(), max_dirty_blocks, d_scratch.data_ptr(),
                                          d_scratch.numel(), _stream_handle(torch)), "snappy_hip_update_ranges")
    return d_scratch


# growing and shrinking one container (snappy_hip_resize)
SEGMENT_DTYPE = np.dtype([("src", "<u8"), ("length", "<u8")])   # snappy_hip_segment


def resize_scratch_bytes(block_size, old_blocks, new_total_len, keep_len, segment_count):
    """Scratch of snappy_hip_resize on the current device (0 for a bad block size)."""
    return int(lib().snappy_hip_resize_scratch_bytes(block_size, old_blocks, new_total_len, keep_len, segment_count))


def make_segments(entries, device="cuda"):
    """entries: list of (src, length) with src a device address (int) -> device tensor of snappy_hip_segment."""
    import torch
    arr = np.zeros(max(len(entries), 1), dtype=SEGMENT_DTYPE)
    for i, (src, length) in enumerate(entries):
        arr[i] = (src, length)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


def resize(d_desc, total_len, block_size, keep_len, new_total_len, d_segments, segment_count, d_segment_status, d_new_stream, d_new_offsets,
           d_new_stream_len, d_result, d_scratch=None, capacity=None):
    """Enqueue snappy_hip_resize on the current stream.  d_desc: make_stream_descs() tensor of ONE descriptor (block_offsets
    filled in), d_segments: make_segments() tensor, d_segment_status: device int32 tensor of segment_count entries,
    d_new_stream: device uint8 tensor (capacity: its size), d_new_offsets: device int64 tensor of num_blocks(new_total_len) + 1
    entries, d_new_stream_len: device int64 tensor of one entry, d_result: device int32 tensor of two.  d_scratch: 256-byte
    aligned device uint8 tensor (default: a fresh one).  Nothing is synchronised."""
    import torch
    if not 0 <= new_total_len <= 0xffffffff or not 0 <= keep_len <= 0xffffffff:
        raise SnappyHipError("snappy_hip_resize: keep_len and new_total_len must fit the format's 32 bits")
    if d_scratch is None:
        d_scratch = torch.empty(resize_scratch_bytes(block_size, num_blocks(total_len, block_size), new_total_len, keep_len, segment_count),
                                dtype=torch.uint8, device=d_new_stream.device)
    _check(lib().snappy_hip_resize(d_desc.data_ptr(), total_len, block_size, keep_len, new_total_len,
                                   d_segments.data_ptr() if segment_count else None, segment_count,
                                   d_segment_status.data_ptr() if segment_count else None, d_new_stream.data_ptr(),
                                   d_new_stream.numel() if capacity is None else capacity, d_new_offsets.data_ptr(),
                                   d_new_stream_len.data_ptr(), d_result.data_ptr(), d_scratch.data_ptr(), d_scratch.numel(),
                                   _stream_handle(torch)), "snappy_hip_resize")
    return d_scratch


# batches of raw Snappy streams, described on the device (snappy_hip_raw_decompress_batch / snappy_hip_raw_compress_batch)
RAW_DST_TOO_SMALL = 5
RAW_TOO_LARGE = 6
RAW_MAX_LEN = 0x7ffff000
RAW_ITEM_DTYPE = np.dtype([("src", "<u8"), ("src_len", "<u8"), ("dst", "<u8"), ("dst_capacity", "<u8")])   # snappy_hip_raw_item


def make_raw_items(entries, device="cuda"):
    """entries: list of (src, src_len, dst, dst_capacity) with src and dst device addresses (int, 0 = null) -> device tensor of
    snappy_hip_raw_item."""
    import torch
    arr = np.zeros(max(len(entries), 1), dtype=RAW_ITEM_DTYPE)
    for i, e in enumerate(entries):
        arr[i] = tuple(e)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


def raw_decompress_batch(d_items, count, d_out_len, d_status):
    """Enqueue snappy_hip_raw_decompress_batch on the current stream.  d_items: make_raw_items() tensor or any device uint8
    tensor of packed snappy_hip_raw_item, d_out_len: device int64 tensor and d_status: device int32 tensor of `count` entries.
    Nothing is synchronised."""
    import torch
    _check(lib().snappy_hip_raw_decompress_batch(d_items.data_ptr(), count, d_out_len.data_ptr(), d_status.data_ptr(), _stream_handle(torch)),
           "snappy_hip_raw_decompress_batch")


def raw_decompress_split_scratch_bytes(count, unit_len, segment_bytes, max_segments, max_units):
    """Scratch of snappy_hip_raw_decompress_split_batch (0 for a bad unit_len or segment_bytes)."""
    return int(lib().snappy_hip_raw_decompress_split_scratch_bytes(count, unit_len, segment_bytes, max_segments, max_units))


def raw_decompress_split_batch(d_items, count, unit_len, segment_bytes, max_segments, max_units, d_out_len, d_status, d_result, d_scratch=None):
    """Enqueue snappy_hip_raw_decompress_split_batch on the current stream: raw_decompress_batch with every large item decoded by
    many wavefronts where it is built from independent pieces of unit_len output bytes (0 = 65,536), serially where not.
    segment_bytes: 0 = the default (16 KiB); max_segments / max_units: what the scratch is sized for.  d_result: device int32 tensor of
    four (split, small, fallen back, 0).  d_scratch: 256-byte aligned device uint8 tensor (default: a fresh one).  Nothing is
    synchronised."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(max(raw_decompress_split_scratch_bytes(count, unit_len, segment_bytes, max_segments, max_units), 256),
                                dtype=torch.uint8, device=d_result.device)
    _check(lib().snappy_hip_raw_decompress_split_batch(d_items.data_ptr() if count else None, count, unit_len, segment_bytes, max_segments, max_units,
                                                       d_out_len.data_ptr() if count else None, d_status.data_ptr() if count else None,
                                                       d_result.data_ptr(), d_scratch.data_ptr(), d_scratch.numel(), _stream_handle(torch)),
           "snappy_hip_raw_decompress_split_batch")
    return d_scratch


def raw_compress_bound(src_len, block_size):
    """A dst_capacity that always suffices for an item of src_len bytes (0 for a bad block size)."""
    return int(lib().snappy_hip_raw_compress_bound(src_len, block_size))


def raw_compress_scratch_bytes(block_size, count, max_fragments):
    """Scratch of snappy_hip_raw_compress_batch (0 for a bad block size)."""
    return int(lib().snappy_hip_raw_compress_scratch_bytes(block_size, count, max_fragments))


def raw_compress_batch(d_items, count, block_size, max_fragments, d_out_len, d_status, d_result, d_scratch=None):
    """Enqueue snappy_hip_raw_compress_batch on the current stream.  d_out_len: device int64 tensor and d_status: device int32
    tensor of `count` entries, d_result: device int32 tensor of two.  d_scratch: 256-byte aligned device uint8 tensor (default: a
    fresh one).  Nothing is synchronised."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(raw_compress_scratch_bytes(block_size, count, max_fragments), dtype=torch.uint8, device=d_result.device)
    _check(lib().snappy_hip_raw_compress_batch(d_items.data_ptr(), count, block_size, max_fragments, d_out_len.data_ptr(),
                                               d_status.data_ptr(), d_result.data_ptr(), d_scratch.data_ptr(), d_scratch.numel(),
                                               _stream_handle(torch)), "snappy_hip_raw_compress_batch")
    return d_scratch


def compress_tables(device=None):
    """A fresh table workspace of the full grid for raw_compress_batch_tables / sz_compress_batch_tables (and compress_blocks):
    snappy_hip_compress_scratch_bytes() bytes, 256-byte aligned, not initialised."""
    import torch
    return torch.empty(int(lib().snappy_hip_compress_scratch_bytes()), dtype=torch.uint8, device=device or "cuda")


def raw_compress_batch_tables(d_items, count, block_size, max_fragments, d_out_len, d_status, d_result, d_tables=None, d_scratch=None):
    """Enqueue snappy_hip_raw_compress_batch_tables on the current stream: raw_compress_batch with the fragments compressed by
    K1's global-table wavefronts.  Arrays as in raw_compress_batch, but d_result has FOUR int32 entries ([2] = the fragments
    global-table wavefronts compressed, [3] = 0).  d_tables: 256-byte aligned device uint8 tensor (default: compress_tables());
    fewer bytes only mean fewer wavefronts, less than one table is refused.  Nothing is synchronised.  -> (d_scratch, d_tables)"""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(max(raw_compress_scratch_bytes(block_size, count, max_fragments), 256), dtype=torch.uint8, device=d_result.device)
    if d_tables is None:
        d_tables = compress_tables(d_result.device)
    _check(lib().snappy_hip_raw_compress_batch_tables(d_items.data_ptr() if count else None, count, block_size, max_fragments,
                                                      d_out_len.data_ptr() if count else None, d_status.data_ptr() if count else None,
                                                      d_result.data_ptr(), d_scratch.data_ptr(), d_scratch.numel(), d_tables.data_ptr(),
                                                      d_tables.numel(), _stream_handle(torch)), "snappy_hip_raw_compress_batch_tables")
    return d_scratch, d_tables


def sz_compress_batch_tables(d_items, count, chunk_len, max_chunks, d_out_len, d_status, d_result, d_tables=None, d_scratch=None):
    """Enqueue snappy_hip_sz_compress_batch_tables on the current stream: sz_compress_batch with the chunks compressed by K1's
    global-table wavefronts.  Arrays and d_tables as in raw_compress_batch_tables.  -> (d_scratch, d_tables)"""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(max(sz_compress_scratch_bytes(chunk_len, count, max_chunks), 256), dtype=torch.uint8, device=d_result.device)
    if d_tables is None:
        d_tables = compress_tables(d_result.device)
    _check(lib().snappy_hip_sz_compress_batch_tables(d_items.data_ptr() if count else None, count, chunk_len, max_chunks,
                                                     d_out_len.data_ptr() if count else None, d_status.data_ptr() if count else None,
                                                     d_result.data_ptr(), d_scratch.data_ptr(), d_scratch.numel(), d_tables.data_ptr(),
                                                     d_tables.numel(), _stream_handle(torch)), "snappy_hip_sz_compress_batch_tables")
    return d_scratch, d_tables


# the Snappy framing format (.sz) and CRC-32C (snappy_hip_sz_decompress_batch / snappy_hip_sz_compress_batch / snappy_hip_crc32c_batch)
SZ_CRC_MISMATCH = 7
SZ_UNSUPPORTED = 8
SZ_NO_VERIFY = 1
CRC_ITEM_DTYPE = np.dtype([("src", "<u8"), ("src_len", "<u8")])   # snappy_hip_crc_item


def make_crc_items(entries, device="cuda"):
    """entries: list of (src, src_len) with src a device address (int, 0 = null) -> device tensor of snappy_hip_crc_item."""
    import torch
    arr = np.zeros(max(len(entries), 1), dtype=CRC_ITEM_DTYPE)
    for i, e in enumerate(entries):
        arr[i] = tuple(e)
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


def crc32c_batch(d_items, count, d_crc):
    """Enqueue snappy_hip_crc32c_batch on the current stream: d_crc[i] (device int32 tensor of `count` entries) = the unmasked
    CRC-32C of item i.  Nothing is synchronised."""
    import torch
    _check(lib().snappy_hip_crc32c_batch(d_items.data_ptr(), count, d_crc.data_ptr(), _stream_handle(torch)), "snappy_hip_crc32c_batch")


def sz_decompress_scratch_bytes(count, max_chunks):
    """Scratch of snappy_hip_sz_decompress_batch."""
    return int(lib().snappy_hip_sz_decompress_scratch_bytes(count, max_chunks))


def sz_decompress_batch(d_items, count, max_chunks, d_out_len, d_status, d_bad_chunk, d_result, flags=0, d_scratch=None):
    """Enqueue snappy_hip_sz_decompress_batch on the current stream.  d_items: make_raw_items() tensor, each src one .sz stream.
    d_out_len: device int64 tensor, d_status and d_bad_chunk: device int32 tensors of `count` entries, d_result: device int32
    tensor of two (chunks the batch needs, items OK).  flags: SZ_NO_VERIFY skips the CRC comparison.  d_scratch: 256-byte
    aligned device uint8 tensor (default: a fresh one).  Nothing is synchronised."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(max(sz_decompress_scratch_bytes(count, max_chunks), 256), dtype=torch.uint8, device=d_result.device)
    _check(lib().snappy_hip_sz_decompress_batch(d_items.data_ptr() if count else None, count, max_chunks, flags, d_out_len.data_ptr() if count else None,
                                                d_status.data_ptr() if count else None, d_bad_chunk.data_ptr() if count else None,
                                                d_result.data_ptr(), d_scratch.data_ptr(), d_scratch.numel(), _stream_handle(torch)),
           "snappy_hip_sz_decompress_batch")
    return d_scratch


def sz_decompress_split_scratch_bytes(count, max_chunks, segment_bytes, max_segments):
    """Scratch of snappy_hip_sz_decompress_split_batch (0 for a bad segment_bytes)."""
    return int(lib().snappy_hip_sz_decompress_split_scratch_bytes(count, max_chunks, segment_bytes, max_segments))


def sz_decompress_split_batch(d_items, count, max_chunks, segment_bytes, max_segments, d_out_len, d_status, d_bad_chunk, d_result, flags=0,
                              d_scratch=None):
    """Enqueue snappy_hip_sz_decompress_split_batch on the current stream: sz_decompress_batch with the chunk chain of every item
    of more than one segment walked by many wavefronts; the same answers.  segment_bytes: 0 = the default (1 MiB); max_segments:
    what the scratch is sized for.  d_result: device int32 tensor of four (chunks the batch needs, items OK, large items the
    parallel walk proved, large items walked serially).  d_scratch: 256-byte aligned device uint8 tensor (default: a fresh one).
    Nothing is synchronised."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(max(sz_decompress_split_scratch_bytes(count, max_chunks, segment_bytes, max_segments), 256), dtype=torch.uint8,
                                device=d_result.device)
    _check(lib().snappy_hip_sz_decompress_split_batch(d_items.data_ptr() if count else None, count, max_chunks, segment_bytes, max_segments, flags,
                                                      d_out_len.data_ptr() if count else None, d_status.data_ptr() if count else None,
                                                      d_bad_chunk.data_ptr() if count else None, d_result.data_ptr(), d_scratch.data_ptr(),
                                                      d_scratch.numel(), _stream_handle(torch)), "snappy_hip_sz_decompress_split_batch")
    return d_scratch


# byte ranges of .sz streams from a resident chunk index (snappy_hip_sz_index_batch / snappy_hip_sz_decompress_ranges)
SZ_CHUNK_DTYPE = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("info", "<u4"), ("ulen", "<u4"), ("item", "<u4"), ("reserved", "<u4")])   # snappy_hip_sz_chunk
SZ_DESC_DTYPE = np.dtype([("src", "<u8"), ("src_len", "<u8"), ("chunks", "<u8"), ("num_chunks", "<u8"), ("total_len", "<u8")])   # snappy_hip_sz_desc


def sz_index_scratch_bytes(count, max_chunks, segment_bytes, max_segments):
    """Scratch of snappy_hip_sz_index_batch (0 for a bad segment_bytes)."""
    return int(lib().snappy_hip_sz_index_scratch_bytes(count, max_chunks, segment_bytes, max_segments))


def sz_index_batch(d_items, count, max_chunks, segment_bytes, max_segments, d_chunks, d_descs, d_status, d_result, d_scratch=None):
    """Enqueue snappy_hip_sz_index_batch on the current stream: the chunk index of `count` .sz streams.  d_items: make_raw_items()
    tensor (dst and capacity are ignored); d_chunks: device uint8 tensor of 32 * max_chunks bytes (SZ_CHUNK_DTYPE), d_descs: of
    40 * count bytes (SZ_DESC_DTYPE); d_status: device int32 tensor of `count`, d_result: of four.  d_scratch: 256-byte aligned
    device uint8 tensor (default: a fresh one).  Nothing is synchronised."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(max(sz_index_scratch_bytes(count, max_chunks, segment_bytes, max_segments), 256), dtype=torch.uint8,
                                device=d_result.device)
    _check(lib().snappy_hip_sz_index_batch(d_items.data_ptr() if count else None, count, max_chunks, segment_bytes, max_segments,
                                           d_chunks.data_ptr() if max_chunks else None, d_descs.data_ptr() if count else None,
                                           d_status.data_ptr() if count else None, d_result.data_ptr(), d_scratch.data_ptr(), d_scratch.numel(),
                                           _stream_handle(torch)), "snappy_hip_sz_index_batch")
    return d_scratch


def sz_decompress_ranges_scratch_bytes(range_count):
    """Scratch for a full grid of snappy_hip_sz_decompress_ranges on the current device."""
    return int(lib().snappy_hip_sz_decompress_ranges_scratch_bytes(range_count))


def sz_decompress_ranges(d_descs, count, d_ranges, range_count, d_status, d_bad_chunk, flags=0, d_scratch=None):
    """Enqueue snappy_hip_sz_decompress_ranges on the current stream.  d_descs: the tensor sz_index_batch filled (or any packed
    SZ_DESC_DTYPE), d_ranges: make_ranges() tensor whose stream field indexes d_descs, d_status and d_bad_chunk: device int32
    tensors of range_count entries.  flags: SZ_NO_VERIFY.  d_scratch: 256-byte aligned device uint8 tensor (default: a fresh one
    for the full grid).  Nothing is synchronised."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(sz_decompress_ranges_scratch_bytes(range_count), dtype=torch.uint8, device=d_status.device)
    _check(lib().snappy_hip_sz_decompress_ranges(d_descs.data_ptr() if count else None, count, d_ranges.data_ptr() if range_count else None,
                                                 range_count, flags, d_status.data_ptr() if range_count else None,
                                                 d_bad_chunk.data_ptr() if range_count else None, d_scratch.data_ptr(), d_scratch.numel(),
                                                 _stream_handle(torch)), "snappy_hip_sz_decompress_ranges")
    return d_scratch


def sz_compress_bound(src_len, chunk_len):
    """10 + 8 * chunks + src_len: a dst_capacity that always suffices, exact when nothing compresses (0 for a bad chunk_len)."""
    return int(lib().snappy_hip_sz_compress_bound(src_len, chunk_len))


def sz_compress_scratch_bytes(chunk_len, count, max_chunks):
    """Scratch of snappy_hip_sz_compress_batch (0 for a bad chunk_len)."""
    return int(lib().snappy_hip_sz_compress_scratch_bytes(chunk_len, count, max_chunks))


def sz_compress_batch(d_items, count, chunk_len, max_chunks, d_out_len, d_status, d_result, d_scratch=None):
    """Enqueue snappy_hip_sz_compress_batch on the current stream: item i's plaintext as one .sz stream of chunk_len chunks.
    Arrays as in raw_compress_batch.  Nothing is synchronised."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(max(sz_compress_scratch_bytes(chunk_len, count, max_chunks), 256), dtype=torch.uint8, device=d_result.device)
    _check(lib().snappy_hip_sz_compress_batch(d_items.data_ptr() if count else None, count, chunk_len, max_chunks,
                                              d_out_len.data_ptr() if count else None, d_status.data_ptr() if count else None, d_result.data_ptr(),
                                              d_scratch.data_ptr(), d_scratch.numel(), _stream_handle(torch)), "snappy_hip_sz_compress_batch")
    return d_scratch


# checking without decoding (snappy_hip_check_blocks, snappy_hip_raw_check_batch)
CHECK_NONE = 0xffffffff


def check_scratch_bytes(count):
    """Scratch of snappy_hip_check_blocks for `count` containers."""
    return int(lib().snappy_hip_check_scratch_bytes(count))


def check_blocks(d_descs, count, d_results, d_block_status=None, d_scratch=None):
    """Enqueue snappy_hip_check_blocks on the current stream.  d_descs: make_stream_descs() tensor (block_offsets filled in; result
    is not touched), d_results: device int32 tensor of 4 * count entries, d_block_status: None, or a device int64 tensor of `count`
    device addresses (0 = no status array for that container).  d_scratch: 256-byte aligned device uint8 tensor (default: a fresh
    one).  Nothing is synchronised."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(max(check_scratch_bytes(count), 256), dtype=torch.uint8, device=d_results.device)
    _check(lib().snappy_hip_check_blocks(d_descs.data_ptr(), count, d_block_status.data_ptr() if d_block_status is not None else None,
                                         d_results.data_ptr(), d_scratch.data_ptr(), d_scratch.numel(), _stream_handle(torch)),
           "snappy_hip_check_blocks")
    return d_scratch


def raw_check_batch(d_items, count, d_out_len, d_status):
    """Enqueue snappy_hip_raw_check_batch on the current stream: as raw_decompress_batch, the items' dst and dst_capacity
    ignored.  Nothing is synchronised."""
    import torch
    _check(lib().snappy_hip_raw_check_batch(d_items.data_ptr(), count, d_out_len.data_ptr(), d_status.data_ptr(), _stream_handle(torch)),
           "snappy_hip_raw_check_batch")


def raw_check_split_scratch_bytes(count, segment_bytes, max_segments):
    """Scratch of snappy_hip_raw_check_split_batch (0 for a bad segment_bytes)."""
    return int(lib().snappy_hip_raw_check_split_scratch_bytes(count, segment_bytes, max_segments))


def raw_check_split_batch(d_items, count, segment_bytes, max_segments, d_out_len, d_status, d_result, d_scratch=None):
    """Enqueue snappy_hip_raw_check_split_batch on the current stream: raw_check_batch with every item of more than one segment
    checked by many wavefronts, whatever built it.  segment_bytes: 0 = the default (16 KiB); max_segments: what the scratch is
    sized for.  d_result: device int32 tensor of four (proven by the parallel path, not large, sent to the serial checker, 0).
    d_scratch: 256-byte aligned device uint8 tensor (default: a fresh one).  Nothing is synchronised."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(max(raw_check_split_scratch_bytes(count, segment_bytes, max_segments), 256), dtype=torch.uint8, device=d_result.device)
    _check(lib().snappy_hip_raw_check_split_batch(d_items.data_ptr() if count else None, count, segment_bytes, max_segments,
                                                  d_out_len.data_ptr() if count else None, d_status.data_ptr() if count else None,
                                                  d_result.data_ptr(), d_scratch.data_ptr(), d_scratch.numel(), _stream_handle(torch)),
           "snappy_hip_raw_check_split_batch")
    return d_scratch


def check_resident(d_stream, stream_len=None):
    """Is the framed stream held in a CUDA uint8 tensor intact?  Indexes it (the size chain), then checks every block without
    decoding it -> (ok, bad_blocks, first_bad_block).  A broken header or chain: (False, 1, the number of blocks the walk
    found); first_bad_block is None when the stream is intact."""
    import torch
    stream_len = d_stream.numel() if stream_len is None else stream_len
    head = bytes(d_stream[:min(10, stream_len)].cpu().numpy())
    total, bs, hdr = parse_header(head)
    if hdr == 0 or (total and not 1 <= bs <= 65535):
        return False, 1, 0
    nb = num_blocks(total, bs) if total else 0
    if nb == 0:
        return (True, 0, None) if stream_len == hdr else (False, 1, 0)
    dev = d_stream.device
    d_boff = torch.empty(nb, dtype=torch.int64, device=dev)
    d_res = torch.full((2,), 7, dtype=torch.int32, device=dev)
    descs = make_stream_descs([dict(stream=d_stream, stream_len=stream_len, block_offsets=d_boff, result=d_res,
                                    total_len=total, block_size=bs, header_len=hdr, num_blocks=nb)], dev)
    index_streams(descs, 1)
    res = d_res.cpu().numpy()
    if res[0] != 0 or res[1] != nb:
        return False, 1, int(res[1]) & 0x7fffffff
    d_results = torch.full((4,), 7, dtype=torch.int32, device=dev)
    check_blocks(descs, 1, d_results)
    r = [int(x) & 0xffffffff for x in d_results.cpu().numpy()]
    if r[0] == 0:
        return True, 0, None
    return False, r[1], (r[2] if r[2] != CHECK_NONE else 0)


# ---------------------------------------------------------------------------
# drop-in pair (host buffers), driven the way dpu_snappy.c's main() drives the *_dpu functions
# ---------------------------------------------------------------------------

def compress_host(data, block_size=32768, out_capacity=None):
    """snappy_compress_gpu on a host buffer -> (status, stream bytes, runtime dict).  out_capacity: hand over a
    caller-owned output buffer of that many bytes (finite `max`) instead of letting the callee allocate."""
    a = np.frombuffer(data, dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    inp = HostBufferContext(b"<memory>", a.ctypes.data, a.ctypes.data, len(data), (1 << 64) - 1)
    if out_capacity is None:
        out = HostBufferContext(b"<memory>", None, None, 0, (1 << 64) - 1)
    else:
        buf = libc().malloc(max(1, out_capacity))
        out = HostBufferContext(b"<memory>", buf, buf, 0, out_capacity)
    rt = ProgramRuntime()
    st = lib().snappy_compress_gpu(ctypes.byref(inp), ctypes.byref(out), block_size, ctypes.byref(rt))
    stream = b""
    if st == SNAPPY_OK:
        stream = ctypes.string_at(out.buffer, out.length)
    if out.buffer:
        libc().free(out.buffer)
    return st, stream, rt.as_dict()


def decompress_host(stream, out_len_override=None):
    """setup_decompression (reference snappy_decompress.c:187-215) + snappy_decompress_gpu -> (status, bytes, runtime).
    out_len_override: bytes to allocate for the plaintext instead of the header's length (tests with hostile headers)."""
    a = np.frombuffer(stream, dtype=np.uint8).copy()
    # first varint: uncompressed length
    total, shift, used = 0, 0, 0
    ok = False
    for k in range(min(5, a.size)):
        c = int(a[k])
        total |= (c & 0x7f) << shift
        used = k + 1
        if not c & 0x80:
            ok = True
            break
        shift += 7
    if not ok:
        return SNAPPY_INVALID_INPUT, b"", {}
    size = (((total + 7) & ~7) | 2047) if out_len_override is None else max(8, out_len_override)
    buf = libc().malloc(size)
    inp = HostBufferContext(b"<memory>", a.ctypes.data, a.ctypes.data + used, a.size, (1 << 64) - 1)
    out = HostBufferContext(b"<memory>", buf, buf, total, (1 << 64) - 1)
    rt = ProgramRuntime()
    st = lib().snappy_decompress_gpu(ctypes.byref(inp), ctypes.byref(out), ctypes.byref(rt))
    plain = ctypes.string_at(out.buffer, total) if st == SNAPPY_OK else b""
    libc().free(buf)
    return st, plain, rt.as_dict()


def decompress_host_wide(stream, waves_per_block=0, out_capacity=None):
    """snappy_decompress_wide_gpu on a whole framed file held in host memory -> (status, bytes, runtime dict), as decompress_host.
    out_capacity: hand over a caller-owned output buffer of that many bytes (finite `max`) instead of letting the callee allocate."""
    a = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, dtype=np.uint8)
    inp = HostBufferContext(b"<memory>", a.ctypes.data, a.ctypes.data, len(stream), (1 << 64) - 1)
    if out_capacity is None:
        out = HostBufferContext(b"<memory>", None, None, 0, (1 << 64) - 1)
    else:
        buf = libc().malloc(max(1, out_capacity))
        out = HostBufferContext(b"<memory>", buf, buf, 0, out_capacity)
    rt = ProgramRuntime()
    st = lib().snappy_decompress_wide_gpu(ctypes.byref(inp), ctypes.byref(out), waves_per_block, ctypes.byref(rt))
    data = ctypes.string_at(out.buffer, out.length) if st == SNAPPY_OK else b""
    if out.buffer:
        libc().free(out.buffer)
    return st, data, rt.as_dict()


def decompress_range_host(stream, offset, length, out_capacity=None):
    """snappy_decompress_range_gpu on a whole framed file held in host memory -> (status, bytes, runtime dict).
    out_capacity: hand over a caller-owned output buffer of that many bytes (finite `max`) instead of letting the callee allocate."""
    a = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, dtype=np.uint8)
    inp = HostBufferContext(b"<memory>", a.ctypes.data, a.ctypes.data, len(stream), (1 << 64) - 1)
    if out_capacity is None:
        out = HostBufferContext(b"<memory>", None, None, 0, (1 << 64) - 1)
    else:
        buf = libc().malloc(max(1, out_capacity))
        out = HostBufferContext(b"<memory>", buf, buf, 0, out_capacity)
    rt = ProgramRuntime()
    st = lib().snappy_decompress_range_gpu(ctypes.byref(inp), ctypes.byref(out), offset, length, ctypes.byref(rt))
    data = ctypes.string_at(out.buffer, out.length) if st == SNAPPY_OK else b""
    if out.buffer:
        libc().free(out.buffer)
    return st, data, rt.as_dict()


def update_range_host(stream, offset, data, out_capacity=None):
    """snappy_update_range_gpu on a whole framed file held in host memory: `data` over plaintext bytes [offset, offset +
    len(data)) -> (status, new stream bytes, runtime dict).  out_capacity: as in compress_host."""
    a = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, dtype=np.uint8)
    b = np.frombuffer(data, dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    inp = HostBufferContext(b"<memory>", a.ctypes.data, a.ctypes.data, len(stream), (1 << 64) - 1)
    patch = HostBufferContext(b"<memory>", b.ctypes.data, b.ctypes.data, len(data), (1 << 64) - 1)
    if out_capacity is None:
        out = HostBufferContext(b"<memory>", None, None, 0, (1 << 64) - 1)
    else:
        buf = libc().malloc(max(1, out_capacity))
        out = HostBufferContext(b"<memory>", buf, buf, 0, out_capacity)
    rt = ProgramRuntime()
    st = lib().snappy_update_range_gpu(ctypes.byref(inp), ctypes.byref(patch), offset, ctypes.byref(out), ctypes.byref(rt))
    new = ctypes.string_at(out.buffer, out.length) if st == SNAPPY_OK else b""
    if out.buffer:
        libc().free(out.buffer)
    return st, new, rt.as_dict()


def resize_host(stream, keep_len, tail=None, out_capacity=None):
    """snappy_resize_gpu on a whole framed file held in host memory: the first keep_len bytes of its plaintext, then `tail`
    (bytes, or None for a NULL tail) -> (status, new stream bytes, runtime dict).  out_capacity: as in compress_host."""
    a = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, dtype=np.uint8)
    inp = HostBufferContext(b"<memory>", a.ctypes.data, a.ctypes.data, len(stream), (1 << 64) - 1)
    tail_ref = None
    if tail is not None:
        b = np.frombuffer(tail, dtype=np.uint8).copy() if len(tail) else np.zeros(1, dtype=np.uint8)
        tail_ctx = HostBufferContext(b"<memory>", b.ctypes.data, b.ctypes.data, len(tail), (1 << 64) - 1)
        tail_ref = ctypes.byref(tail_ctx)
    if out_capacity is None:
        out = HostBufferContext(b"<memory>", None, None, 0, (1 << 64) - 1)
    else:
        buf = libc().malloc(max(1, out_capacity))
        out = HostBufferContext(b"<memory>", buf, buf, 0, out_capacity)
    rt = ProgramRuntime()
    st = lib().snappy_resize_gpu(ctypes.byref(inp), keep_len, tail_ref, ctypes.byref(out), ctypes.byref(rt))
    new = ctypes.string_at(out.buffer, out.length) if st == SNAPPY_OK else b""
    if out.buffer:
        libc().free(out.buffer)
    return st, new, rt.as_dict()


def _raw_host(call, data, out_capacity):
    a = np.frombuffer(data, dtype=np.uint8).copy() if len(data) else np.zeros(1, dtype=np.uint8)
    inp = HostBufferContext(b"<memory>", a.ctypes.data, a.ctypes.data, len(data), (1 << 64) - 1)
    if out_capacity is None:
        out = HostBufferContext(b"<memory>", None, None, 0, (1 << 64) - 1)
    else:
        buf = libc().malloc(max(1, out_capacity))
        out = HostBufferContext(b"<memory>", buf, buf, 0, out_capacity)
    rt = ProgramRuntime()
    st = call(ctypes.byref(inp), ctypes.byref(out), ctypes.byref(rt))
    got = ctypes.string_at(out.buffer, out.length) if st == SNAPPY_OK else b""
    if out.buffer:
        libc().free(out.buffer)
    return st, got, rt.as_dict()


def raw_compress_host(data, block_size=32768, out_capacity=None):
    """snappy_compress_raw_gpu on a host buffer -> (status, raw Snappy stream, runtime dict).  out_capacity: as in compress_host."""
    return _raw_host(lambda i, o, r: lib().snappy_compress_raw_gpu(i, o, block_size, r), data, out_capacity)


def raw_compress_tables_host(data, block_size=32768, out_capacity=None):
    """snappy_compress_raw_tables_gpu on a host buffer -> (status, raw Snappy stream, runtime dict): raw_compress_host's bytes."""
    return _raw_host(lambda i, o, r: lib().snappy_compress_raw_tables_gpu(i, o, block_size, r), data, out_capacity)


def sz_compress_tables_host(data, chunk_len=32768, out_capacity=None):
    """snappy_compress_sz_tables_gpu on a host buffer -> (status, .sz stream, runtime dict): sz_compress_host's bytes."""
    return _raw_host(lambda i, o, r: lib().snappy_compress_sz_tables_gpu(i, o, chunk_len, r), data, out_capacity)


def raw_decompress_host(stream, out_capacity=None):
    """snappy_decompress_raw_gpu on a whole raw Snappy stream held in host memory -> (status, plaintext, runtime dict)."""
    return _raw_host(lambda i, o, r: lib().snappy_decompress_raw_gpu(i, o, r), stream, out_capacity)


def sz_compress_host(data, chunk_len=32768, out_capacity=None):
    """snappy_compress_sz_gpu on a host buffer -> (status, .sz stream, runtime dict).  out_capacity: as in compress_host."""
    return _raw_host(lambda i, o, r: lib().snappy_compress_sz_gpu(i, o, chunk_len, r), data, out_capacity)


def sz_decompress_host(stream, flags=0, out_capacity=None):
    """snappy_decompress_sz_gpu on a whole .sz stream held in host memory -> (status, plaintext, runtime dict)."""
    return _raw_host(lambda i, o, r: lib().snappy_decompress_sz_gpu(i, o, flags, r), stream, out_capacity)


def sz_decompress_split_host(stream, flags=0, out_capacity=None):
    """snappy_decompress_sz_split_gpu on a whole .sz stream held in host memory -> (status, plaintext, runtime dict)."""
    return _raw_host(lambda i, o, r: lib().snappy_decompress_sz_split_gpu(i, o, flags, r), stream, out_capacity)


def check_host(stream):
    """snappy_check_gpu on a whole framed file held in host memory -> (status, report dict, runtime dict)."""
    a = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, dtype=np.uint8)
    inp = HostBufferContext(b"<memory>", a.ctypes.data, a.ctypes.data, len(stream), (1 << 64) - 1)
    rep, rt = CheckReport(), ProgramRuntime()
    st = lib().snappy_check_gpu(ctypes.byref(inp), ctypes.byref(rep), ctypes.byref(rt))
    return st, rep.as_dict(), rt.as_dict()


def raw_decompress_split_host(stream, unit_len=0, out_capacity=None):
    """snappy_decompress_raw_split_gpu on a whole raw Snappy stream held in host memory -> (status, plaintext, runtime dict)."""
    return _raw_host(lambda i, o, r: lib().snappy_decompress_raw_split_gpu(i, o, unit_len, r), stream, out_capacity)


def check_raw_host(stream, split=False):
    """snappy_check_raw_gpu -- split: snappy_check_raw_split_gpu -- on a whole raw Snappy stream held in host memory -> (status,
    uncompressed length, runtime dict)."""
    a = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, dtype=np.uint8)
    inp = HostBufferContext(b"<memory>", a.ctypes.data, a.ctypes.data, len(stream), (1 << 64) - 1)
    length, rt = ctypes.c_uint64(0), ProgramRuntime()
    st = (lib().snappy_check_raw_split_gpu if split else lib().snappy_check_raw_gpu)(ctypes.byref(inp), ctypes.byref(length), ctypes.byref(rt))
    return st, int(length.value), rt.as_dict()


def check_raw_split_host(stream):
    """snappy_check_raw_split_gpu on a whole raw Snappy stream held in host memory -> (status, uncompressed length, runtime dict)."""
    return check_raw_host(stream, split=True)


def sz_decompress_range_host(stream, offset, length, flags=0, out_capacity=None):
    """snappy_decompress_sz_range_gpu on a whole .sz stream held in host memory -> (status, the range's bytes, runtime dict)."""
    return _raw_host(lambda i, o, r: lib().snappy_decompress_sz_range_gpu(i, o, offset, length, flags, r), stream, out_capacity)
