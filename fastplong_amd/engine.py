"""Python front end of libfastplong_amd.so (the HIP library behind include/fastplong_amd.h).

There is no fallback of any kind: if the library has not been built, or no MI355X is visible,
construction raises.  torch is used only as plumbing (device memory, streams, collectives)."""
import ctypes as C
import os

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libfastplong_amd.so")

# A context drives five streams; the HIP runtime's default is four hardware queues per device, and two streams on one queue run in
# submission order.  The HOST asks for more, before its first HIP call (the library leaves the environment alone).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

EXPORTS = [
    "fpl_abi_version", "fpl_strerror", "fpl_last_error", "fpl_options_default", "fpl_create", "fpl_destroy",
    "fpl_process_batch_device", "fpl_process_batch", "fpl_max_cycles", "fpl_n_adapters", "fpl_counters_len",
    "fpl_reserve_cycles", "fpl_counters_device_ptr", "fpl_get_counters", "fpl_reset_counters", "fpl_synchronize",
    "fpl_enable_timing", "fpl_get_kernel_times", "fpl_fragment_counts", "fpl_get_fragments",
    "fpl_process_batch_async", "fpl_wait", "fpl_in_flight", "fpl_host_alloc", "fpl_host_free", "fpl_allreduce_counters",
    "fpl_count_end_kmers", "fpl_pick_adapter", "fpl_rccl_library", "fpl_comm_init", "fpl_get_batch_forms", "fpl_assume_inputs_ready",
    "fpl_process_text_async", "fpl_wait_text", "fpl_peek_text", "fpl_start_text", "fpl_cancel_text",
    "fpl_set_text_gzip", "fpl_wait_text_gz", "fpl_get_gzip_batches",
    "fpl_process_bam_async", "fpl_decode_bam", "fpl_set_bam_gzip", "fpl_wait_bam_gz", "fpl_set_gzip_framing", "fpl_set_gzip_records",
    "fpl_set_bam_tags", "fpl_get_bam_tag_stats", "fpl_set_bam_mods", "fpl_get_bam_mod_stats",
    "fpl_set_bam_moves", "fpl_get_bam_move_stats",
    "fpl_set_bam_comments", "fpl_get_bam_comment_stats",
    "fpl_inflater_create", "fpl_inflate_bgzf", "fpl_inflater_destroy", "fpl_inflate_gzip",
    "fpl_emit_batch_device", "fpl_set_fragment_output", "fpl_set_emit_break_no",
    "fpl_process_bgzf_bam_async", "fpl_peek_bgzf_bam", "fpl_start_bgzf_bam", "fpl_wait_bgzf_bam", "fpl_bam_tail_get", "fpl_bam_tail_set",
    "fpl_resume_bgzf_bam", "fpl_reserve_bam_tail",
    "fpl_process_bgzf_text_async", "fpl_peek_bgzf_text", "fpl_start_bgzf_text", "fpl_wait_bgzf_text",
]


class FplError(RuntimeError):
    pass


_lib = None


def load_library(path=None):
    """dlopen the in-tree HIP library and declare its prototypes; raises if it is missing.
    path: another build of the same library (tools/ab_bench.py compares kernel variants side by side); not cached."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # torch first: PyTorch-ROCm carries its own libamdhip64; loading ours afterwards makes the
    # dynamic loader resolve to that same runtime, so device pointers and streams are shared.
    # (Loading the system HIP runtime before torch leaves two runtimes in one process.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib_path = path or LIB_PATH
    if not os.path.exists(lib_path):
        raise FplError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback" % lib_path)
    L = C.CDLL(lib_path)
    L.fpl_abi_version.restype = C.c_int
    L.fpl_strerror.restype = C.c_char_p
    L.fpl_strerror.argtypes = [C.c_int]
    L.fpl_last_error.restype = C.c_char_p
    L.fpl_last_error.argtypes = [C.c_void_p]
    L.fpl_options_default.restype = None
    L.fpl_options_default.argtypes = [C.POINTER(abi.FplOptions)]
    L.fpl_create.restype = C.c_int
    L.fpl_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(abi.FplOptions), C.c_char_p, C.c_int32, C.c_char_p,
                             C.c_int32, C.POINTER(abi.FplAdapter), C.c_int32, C.c_int32, C.c_uint32]
    L.fpl_destroy.restype = None
    L.fpl_destroy.argtypes = [C.c_void_p]
    L.fpl_process_batch_device.restype = C.c_int
    L.fpl_process_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                           C.c_uint32, C.c_void_p, C.c_void_p]
    L.fpl_process_batch.restype = C.c_int
    L.fpl_process_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.fpl_max_cycles.restype = C.c_uint32
    L.fpl_max_cycles.argtypes = [C.c_void_p]
    L.fpl_n_adapters.restype = C.c_int32
    L.fpl_n_adapters.argtypes = [C.c_void_p]
    L.fpl_counters_len.restype = C.c_size_t
    L.fpl_counters_len.argtypes = [C.c_void_p]
    L.fpl_reserve_cycles.restype = C.c_int
    L.fpl_reserve_cycles.argtypes = [C.c_void_p, C.c_uint32]
    L.fpl_counters_device_ptr.restype = C.c_void_p
    L.fpl_counters_device_ptr.argtypes = [C.c_void_p]
    L.fpl_get_counters.restype = C.c_int
    L.fpl_get_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.fpl_reset_counters.restype = C.c_int
    L.fpl_reset_counters.argtypes = [C.c_void_p]
    L.fpl_synchronize.restype = C.c_int
    L.fpl_synchronize.argtypes = [C.c_void_p]
    L.fpl_enable_timing.restype = C.c_int
    L.fpl_enable_timing.argtypes = [C.c_void_p, C.c_int]
    L.fpl_get_kernel_times.restype = C.c_int
    L.fpl_get_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                       C.POINTER(C.c_int)]
    L.fpl_fragment_counts.restype = C.c_int
    L.fpl_fragment_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.fpl_get_fragments.restype = C.c_int
    L.fpl_get_fragments.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.fpl_process_batch_async.restype = C.c_int
    L.fpl_process_batch_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.fpl_wait.restype = C.c_int
    L.fpl_wait.argtypes = [C.c_void_p]
    L.fpl_in_flight.restype = C.c_int
    L.fpl_in_flight.argtypes = [C.c_void_p]
    L.fpl_host_alloc.restype = C.c_void_p
    L.fpl_host_alloc.argtypes = [C.c_size_t]
    L.fpl_host_free.restype = None
    L.fpl_host_free.argtypes = [C.c_void_p]
    L.fpl_allreduce_counters.restype = C.c_int
    L.fpl_allreduce_counters.argtypes = [C.POINTER(C.c_void_p), C.c_int32]
    L.fpl_comm_init.restype = C.c_int
    L.fpl_comm_init.argtypes = [C.POINTER(C.c_void_p), C.c_int32]
    L.fpl_assume_inputs_ready.restype = C.c_int
    L.fpl_assume_inputs_ready.argtypes = [C.c_void_p, C.c_int]
    L.fpl_get_batch_forms.restype = C.c_int
    L.fpl_get_batch_forms.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.fpl_rccl_library.restype = C.c_char_p
    L.fpl_rccl_library.argtypes = []
    L.fpl_count_end_kmers.restype = C.c_int
    L.fpl_count_end_kmers.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.POINTER(C.c_uint64)]
    L.fpl_pick_adapter.restype = C.c_int
    L.fpl_pick_adapter.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_int32,
                                   C.POINTER(abi.FplAdapterPick)]
    L.fpl_process_text_async.restype = C.c_int
    L.fpl_process_text_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.fpl_peek_text.restype = C.c_int
    L.fpl_peek_text.argtypes = [C.c_void_p, C.POINTER(abi.FplTextResult)]
    L.fpl_start_text.restype = C.c_int
    L.fpl_start_text.argtypes = [C.c_void_p]
    L.fpl_cancel_text.restype = C.c_int
    L.fpl_cancel_text.argtypes = [C.c_void_p]
    L.fpl_wait_text.restype = C.c_int
    L.fpl_wait_text.argtypes = [C.c_void_p, C.POINTER(abi.FplTextResult), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    if hasattr(L, "fpl_wait_text_gz"):  # (ABI v9; a stand-in library without the gzip calls still loads: gzip=True then raises)
        L.fpl_set_text_gzip.restype = C.c_int
        L.fpl_set_text_gzip.argtypes = [C.c_void_p, C.c_int]
        L.fpl_wait_text_gz.restype = C.c_int
        L.fpl_wait_text_gz.argtypes = [C.c_void_p, C.POINTER(abi.FplTextResult), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.fpl_get_gzip_batches.restype = C.c_int
        L.fpl_get_gzip_batches.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.fpl_process_bam_async.restype = C.c_int
    L.fpl_process_bam_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    L.fpl_decode_bam.restype = C.c_int
    L.fpl_decode_bam.argtypes = [C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    if hasattr(L, "fpl_wait_bam_gz"):  # (ABI v10; as above: without them submit_bam(gzip=True) raises)
        L.fpl_set_bam_gzip.restype = C.c_int
        L.fpl_set_bam_gzip.argtypes = [C.c_void_p, C.c_int]
        L.fpl_wait_bam_gz.restype = C.c_int
        L.fpl_wait_bam_gz.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    if hasattr(L, "fpl_set_gzip_framing"):  # (found by name: without it Engine.set_gzip_framing raises)
        L.fpl_set_gzip_framing.restype = C.c_int
        L.fpl_set_gzip_framing.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "fpl_set_gzip_records"):  # (found by name: without it Engine.set_gzip_records raises)
        L.fpl_set_gzip_records.restype = C.c_int
        L.fpl_set_gzip_records.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "fpl_set_bam_tags"):  # (found by name: without them Engine.set_bam_tags / bam_tag_stats raise)
        L.fpl_set_bam_tags.restype = C.c_int
        L.fpl_set_bam_tags.argtypes = [C.c_void_p, C.c_int]
        L.fpl_get_bam_tag_stats.restype = C.c_int
        L.fpl_get_bam_tag_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    if hasattr(L, "fpl_set_bam_comments"):  # (the same for Engine.set_bam_comments / bam_comment_stats)
        L.fpl_set_bam_comments.restype = C.c_int
        L.fpl_set_bam_comments.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.fpl_get_bam_comment_stats.restype = C.c_int
        L.fpl_get_bam_comment_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    if hasattr(L, "fpl_set_bam_mods"):  # (the same for Engine.set_bam_mods / bam_mod_stats)
        L.fpl_set_bam_mods.restype = C.c_int
        L.fpl_set_bam_mods.argtypes = [C.c_void_p, C.c_int]
        L.fpl_get_bam_mod_stats.restype = C.c_int
        L.fpl_get_bam_mod_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    if hasattr(L, "fpl_set_bam_moves"):  # (the same for Engine.set_bam_moves / bam_move_stats)
        L.fpl_set_bam_moves.restype = C.c_int
        L.fpl_set_bam_moves.argtypes = [C.c_void_p, C.c_int]
        L.fpl_get_bam_move_stats.restype = C.c_int
        L.fpl_get_bam_move_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    if hasattr(L, "fpl_inflate_bgzf"):  # (found by name, the ABI version is still 10: without them Inflater raises)
        L.fpl_inflater_create.restype = C.c_void_p
        L.fpl_inflater_create.argtypes = [C.c_int32]
        L.fpl_inflate_bgzf.restype = C.c_int
        L.fpl_inflate_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
        L.fpl_inflater_destroy.restype = None
        L.fpl_inflater_destroy.argtypes = [C.c_void_p]
    if hasattr(L, "fpl_inflate_gzip"):
        L.fpl_inflate_gzip.restype = C.c_int
        L.fpl_inflate_gzip.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64,
                                       C.c_uint32, C.c_void_p]
    if hasattr(L, "fpl_emit_batch_device"):  # (found by name as well: without it Engine.emit_device raises)
        L.fpl_emit_batch_device.restype = C.c_int
        L.fpl_emit_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "fpl_set_fragment_output"):  # (found by name: without it Engine.set_fragment_output raises)
        L.fpl_set_fragment_output.restype = C.c_int
        L.fpl_set_fragment_output.argtypes = [C.c_void_p, C.c_int]
        L.fpl_set_emit_break_no.restype = C.c_int
        L.fpl_set_emit_break_no.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, "fpl_process_bgzf_bam_async"):  # (found by name too: without them Engine.submit_bgzf raises)
        L.fpl_process_bgzf_bam_async.restype = C.c_int
        L.fpl_process_bgzf_bam_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64]
        L.fpl_peek_bgzf_bam.restype = C.c_int
        L.fpl_peek_bgzf_bam.argtypes = [C.c_void_p, C.c_void_p]
        L.fpl_start_bgzf_bam.restype = C.c_int
        L.fpl_start_bgzf_bam.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.fpl_wait_bgzf_bam.restype = C.c_int
        L.fpl_wait_bgzf_bam.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.fpl_bam_tail_get.restype = C.c_int
        L.fpl_bam_tail_get.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.fpl_bam_tail_set.restype = C.c_int
        L.fpl_bam_tail_set.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.fpl_resume_bgzf_bam.restype = C.c_int
        L.fpl_resume_bgzf_bam.argtypes = [C.c_void_p]
        L.fpl_reserve_bam_tail.restype = C.c_int
        L.fpl_reserve_bam_tail.argtypes = [C.c_void_p, C.c_uint64]
    if hasattr(L, "fpl_process_bgzf_text_async"):  # (found by name too: without them Engine.submit_bgzf_text raises)
        L.fpl_process_bgzf_text_async.restype = C.c_int
        L.fpl_process_bgzf_text_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
        L.fpl_peek_bgzf_text.restype = C.c_int
        L.fpl_peek_bgzf_text.argtypes = [C.c_void_p, C.c_void_p]
        L.fpl_start_bgzf_text.restype = C.c_int
        L.fpl_start_bgzf_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.fpl_wait_bgzf_text.restype = C.c_int
        L.fpl_wait_bgzf_text.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    if L.fpl_abi_version() != abi.FPL_ABI_VERSION:
        raise FplError("ABI version mismatch")
    if path is None:
        _lib = L
    return L


def decode_bam(device, bam, rec_start, off):
    """fpl_decode_bam (no context): inflated BAM record bytes, record starts, output CSR offsets -> (bases, qualities)"""
    L = load_library()
    bam = np.ascontiguousarray(bam, dtype=np.uint8)
    rec_start = np.ascontiguousarray(rec_start, dtype=np.uint64)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    total = int(off[-1]) if n >= 0 and len(off) else 0
    seq = np.zeros(max(total, 1), np.uint8)
    qual = np.zeros(max(total, 1), np.uint8)
    rc = L.fpl_decode_bam(int(device), bam.ctypes.data, len(bam), rec_start.ctypes.data, off.ctypes.data, max(n, 0), seq.ctypes.data,
                          qual.ctypes.data)
    if rc != abi.FPL_OK:
        raise FplError("fpl_decode_bam: %s" % L.fpl_strerror(rc).decode())
    return seq[:total], qual[:total]


class Inflater:
    """One fpl_inflater: BGZF blocks inflated on a device, without a context (fpl_inflate_bgzf)."""

    def __init__(self, device=0, lib=None):
        self.L = lib if lib is not None else load_library()
        if not hasattr(self.L, "fpl_inflate_bgzf"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_inflate_bgzf")
        self.h = self.L.fpl_inflater_create(int(device))
        if not self.h:
            raise FplError("fpl_inflater_create: %s" % self.L.fpl_strerror(abi.FPL_ERR_NO_DEVICE).decode())

    def inflate(self, comp, blocks, out=None):
        """comp: the payloads (uint8); blocks: an array of abi.BGZF_BLOCK_DTYPE (comp_off, out_off, comp_len, isize, crc32).
        out: the buffer the blocks' ranges are written into (bytes outside them are left alone); made here, zeroed and as long
        as the furthest range, when not given.  -> (out, status): status[i] 0 = block i inflated, size and CRC-32 agree."""
        comp = np.ascontiguousarray(comp, dtype=np.uint8)
        blk = np.array(blocks, dtype=np.dtype(abi.BGZF_BLOCK_DTYPE), copy=True, ndmin=1)
        if out is None:
            end = int((blk["out_off"] + blk["isize"]).max()) if len(blk) else 0
            out = np.zeros(end, np.uint8)
        if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("out must be a writable contiguous uint8 array")
        rc = self.L.fpl_inflate_bgzf(self.h, comp.ctypes.data if len(comp) else None, len(comp), blk.ctypes.data if len(blk) else None,
                                     len(blk), out.ctypes.data if len(out) else None, len(out))
        if rc != abi.FPL_OK:
            raise FplError("fpl_inflate_bgzf: %s" % self.L.fpl_strerror(rc).decode())
        return out, blk["status"].copy()

    def inflate_gzip(self, comp, start_bit=0, zdict=b"", out_cap=0, chunk_bytes=0):
        """One window of a member's raw deflate payload through fpl_inflate_gzip: comp (bytes), the bit offset of a block start
        in it, the up to 32 KiB in front of that point.  -> (rc, a record of abi.GZIP_WINDOW_DTYPE, the bytes); rc != 0: the call
        refused its arguments or failed, nothing else is meaningful."""
        if not hasattr(self.L, "fpl_inflate_gzip"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_inflate_gzip")
        comp = np.frombuffer(bytes(comp), np.uint8)
        zd = np.frombuffer(bytes(zdict), np.uint8)
        out = np.zeros(int(out_cap), np.uint8)
        res = np.zeros(1, np.dtype(abi.GZIP_WINDOW_DTYPE))
        rc = self.L.fpl_inflate_gzip(self.h, comp.ctypes.data if len(comp) else None, len(comp), int(start_bit), zd.ctypes.data if len(zd) else None,
                                     len(zd), out.ctypes.data if len(out) else None, len(out), int(chunk_bytes), res.ctypes.data)
        r = res[0]
        ok = rc == abi.FPL_OK and r["status"] == abi.FPL_GZIP_OK
        return rc, r, out[:int(r["out_bytes"])].tobytes() if ok else b""

    def close(self):
        if self.h:
            self.L.fpl_inflater_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _b(s):
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


class BgzfBatch:
    """One submission of Engine.submit_bgzf.  Batches are collected in the order of submission, each through its own wait()."""

    WINDOW = abi.BAM_WINDOW_DTYPE
    OK = abi.FPL_BAMW_OK
    PEEK, START, WAIT = "fpl_peek_bgzf_bam", "fpl_start_bgzf_bam", "fpl_wait_bgzf_bam"

    def __init__(self, eng, gzip, keep):
        self.eng, self.gzip, self._keep = eng, gzip, keep
        self._outs = None

    @classmethod
    def _info(cls, win):
        return {k: int(win[0][k]) for k, _ in cls.WINDOW}

    def peek(self):
        """fpl_peek_bgzf_bam (fpl_peek_bgzf_text): the walk's header as a dict (this must be the oldest BGZF batch that is not started)"""
        win = np.zeros(1, np.dtype(self.WINDOW))
        self.eng._check(getattr(self.eng.L, self.PEEK)(self.eng.h, win.ctypes.data), self.PEEK)
        return self._info(win)

    def wait(self, want_reads=True, seq_out=None, qual_out=None):
        """-> (header dict, records, names as a list of bytes, bases, qualities, gzip member).  want_reads=False: the decoded arrays
        stay on the device and bases / qualities are None; the member is None unless the batch was submitted with gzip=True.  A
        refused batch gives its header and nothing else.  seq_out / qual_out: uint8 pinned_array views the decoded reads land in
        (bases / qualities are then views of them) -- a caller that streams a file gives the same pair again once it is done
        with a batch, and a pair that is too short for this batch is FplError; without them the batch makes a pair of its own,
        which is freed when the returned arrays are dropped."""
        e = self.eng
        if (seq_out is None) != (qual_out is None):
            raise FplError("BgzfBatch.wait: seq_out and qual_out go together")
        if want_reads and self._outs is None:
            h = self.peek()
            if h["status"] == self.OK and h["n_reads"]:
                if seq_out is not None:
                    if min(len(seq_out), len(qual_out)) < h["n_bases"] or seq_out.dtype != np.uint8 or qual_out.dtype != np.uint8:
                        raise FplError("BgzfBatch.wait: seq_out / qual_out are uint8 arrays of at least n_bases = %d bytes" % h["n_bases"])
                    self._outs = (seq_out, qual_out)
                else:
                    self._outs = (e.pinned_array(h["n_bases"] + 1, keep=False), e.pinned_array(h["n_bases"] + 1, keep=False))
                e._check(getattr(e.L, self.START)(e.h, self._outs[0].ctypes.data, self._outs[1].ctypes.data), self.START)
        win = np.zeros(1, np.dtype(self.WINDOW))
        rp, npp, op, gp, gl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        e._check(getattr(e.L, self.WAIT)(e.h, win.ctypes.data, C.byref(rp), C.byref(npp), C.byref(op), C.byref(gp) if self.gzip else None,
                                         C.byref(gl) if self.gzip else None), self.WAIT)
        self._keep = None
        h = self._info(win)
        member = (C.string_at(gp.value, gl.value) if gl.value else b"") if self.gzip else None
        n = h["n_reads"]
        if h["status"] != self.OK or n == 0:
            return h, np.zeros(0, dtype=abi.RESULT_DTYPE), [], None, None, member
        res = np.ctypeslib.as_array(C.cast(rp, C.POINTER(C.c_uint8)), shape=(n * 36,)).view(abi.RESULT_DTYPE).copy()
        off = np.ctypeslib.as_array(C.cast(op, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        blob = C.string_at(npp.value, h["name_bytes"]) if h["name_bytes"] else b""
        names = [blob[int(off[i]):int(off[i + 1])] for i in range(n)]
        seq = qual = None
        if self._outs is not None:
            seq, qual = self._outs[0][:h["n_bases"]], self._outs[1][:h["n_bases"]]
        return h, res, names, seq, qual, member


class BgzfTextBatch(BgzfBatch):
    """One submission of Engine.submit_bgzf_text: BgzfBatch's peek() and wait() over the calls and the header of the BGZF text
    path.  wait() -> (header dict of abi.TEXT_WINDOW_DTYPE, records, names -- every read's whole first line, '@' included --,
    bases, qualities, gzip member); bases and qualities are a CSR pair, read i at the running sum of the reads' lengths."""
    WINDOW = abi.TEXT_WINDOW_DTYPE
    OK = abi.FPL_TXTW_OK
    PEEK, START, WAIT = "fpl_peek_bgzf_text", "fpl_start_bgzf_text", "fpl_wait_bgzf_text"


class Engine:
    """One fpl_ctx on one device."""

    def __init__(self, opt=None, start_adapter="", end_adapter="", fasta=(), device=0, max_cycles=1024, lib=None):
        self.L = lib if lib is not None else load_library()
        self.opt = opt if opt is not None else abi.FplOptions.default()
        self.start, self.end = _b(start_adapter), _b(end_adapter)
        self.fasta = [_b(a) for a in fasta]
        arr = (abi.FplAdapter * max(1, len(self.fasta)))()
        for i, a in enumerate(self.fasta):
            arr[i].seq, arr[i].len = a, len(a)
        h = C.c_void_p()
        rc = self.L.fpl_create(C.byref(h), C.byref(self.opt), self.start, len(self.start), self.end, len(self.end),
                               arr, len(self.fasta), device, max_cycles)
        if rc != 0:
            raise FplError("fpl_create: %s" % self.L.fpl_strerror(rc).decode())
        self.h = h
        self.device = device
        self._bam_gz_on = False   # the context's fpl_set_bam_gzip switch as this front end last set it
        self._bam_gz_flags = []   # one entry per CSR / BAM batch in flight, oldest first: submitted with gzip=True?

    def _check(self, rc, what):
        if rc != 0:
            raise FplError("%s: %s (%s)" % (what, self.L.fpl_strerror(rc).decode(),
                                            (self.L.fpl_last_error(self.h) or b"").decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.fpl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_adapters(self):
        return 2 + len(self.fasta)

    @property
    def max_cycles(self):
        return int(self.L.fpl_max_cycles(self.h))

    def reserve_cycles(self, c):
        self._check(self.L.fpl_reserve_cycles(self.h, int(c)), "fpl_reserve_cycles")

    def process_host(self, seq, qual, off):
        """fpl_process_batch: host numpy buffers in, structured result array out."""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        res = np.zeros(max(n, 1), dtype=abi.RESULT_DTYPE)
        if seq.size == 0:
            seq = np.zeros(1, np.uint8)
            qual = np.zeros(1, np.uint8)
        self._check(self.L.fpl_process_batch(self.h, seq.ctypes.data, qual.ctypes.data, off.ctypes.data, n,
                                             res.ctypes.data), "fpl_process_batch")
        return res[:n]

    def submit_host(self, seq, qual, off, res):
        """fpl_process_batch_async: the arrays (uint8, uint8, uint64 offsets; ideally views of pinned_array()) and
        the result array must stay alive until wait() has returned for this batch"""
        n = len(off) - 1
        self._check(self.L.fpl_process_batch_async(self.h, seq.ctypes.data, qual.ctypes.data, off.ctypes.data, n,
                                                   res.ctypes.data), "fpl_process_batch_async")
        self._bam_gz_flags.append(False)

    def wait(self, member=True):
        """fpl_wait for the oldest CSR / BAM batch -> None; for a batch submitted with submit_bam(gzip=True) fpl_wait_bam_gz -> the
        batch's gzip member as bytes (b"" when no read passed).  member=False: plain fpl_wait for such a batch too -- its bytes are
        then never made."""
        want = bool(member and self._bam_gz_flags and self._bam_gz_flags[0])
        gp, gl = C.c_void_p(), C.c_uint64(0)
        rc = self.L.fpl_wait_bam_gz(self.h, C.byref(gp), C.byref(gl)) if want else self.L.fpl_wait(self.h)
        # FPL_ERR_STATE / FPL_ERR_ARG: nothing was collected (nothing in flight, or a text batch is the oldest) and the library's
        # queue is as it was; after any other outcome the batch has left it
        if rc not in (abi.FPL_ERR_STATE, abi.FPL_ERR_ARG) and self._bam_gz_flags:
            self._bam_gz_flags.pop(0)
        self._check(rc, "fpl_wait_bam_gz" if want else "fpl_wait")
        if not want:
            return None
        return C.string_at(gp.value, gl.value) if gl.value else b""

    def submit_bam(self, bam, rec_start, off, seq_out=None, qual_out=None, res=None, gzip=False):
        """fpl_process_bam_async: inflated BAM record bytes (uint8, with at least one addressable byte), where each record
        starts (uint64), the output CSR offsets (uint64, n + 1); the decoded bases and qualities land in seq_out / qual_out
        (pinned_array views of >= off[-1] bytes) and the records in res.  Everything must stay alive until wait().
        gzip=True: the passing reads also come back as a gzip member, composed and deflated on the device -- wait() returns it;
        seq_out / qual_out may then both be None, and the decoded arrays stay on the device."""
        n = len(off) - 1
        if res is None:
            raise FplError("submit_bam: res is required")
        if (seq_out is None) != (qual_out is None) or (seq_out is None and not gzip):
            raise FplError("submit_bam: seq_out and qual_out may be left out only together, and only with gzip=True")
        if gzip or self._bam_gz_on:  # (the switch is the context's: touched only when it has to change)
            if not hasattr(self.L, "fpl_wait_bam_gz"):
                raise FplError("gzip=True needs fpl_set_bam_gzip / fpl_wait_bam_gz (C-ABI version 10)")
            self._check(self.L.fpl_set_bam_gzip(self.h, int(bool(gzip))), "fpl_set_bam_gzip")
            self._bam_gz_on = bool(gzip)
        self._keep_bam = (getattr(self, "_keep_bam", []) + [(bam, rec_start, off)])[-(abi.FPL_MAX_IN_FLIGHT + 1):]
        self._check(self.L.fpl_process_bam_async(self.h, bam.ctypes.data, len(bam), rec_start.ctypes.data, off.ctypes.data, n,
                                                 seq_out.ctypes.data if seq_out is not None else None,
                                                 qual_out.ctypes.data if qual_out is not None else None, res.ctypes.data),
                    "fpl_process_bam_async")
        self._bam_gz_flags.append(bool(gzip))

    def submit_bgzf(self, comp, blocks, skip=0, gzip=False):
        """fpl_process_bgzf_bam_async: the payloads of a BAM's BGZF blocks (uint8, ideally a pinned_array view) and their
        descriptors (abi.BGZF_BLOCK_DTYPE; fastplong_amd.bgzf.blocks cuts a file into them), `skip` inflated bytes in front of
        the first record (the first submission of a file only).  Inflate, record walk, decode and the per-read kernels all run
        on the device -> a BgzfBatch with peek() and wait().  The batch keeps `comp` alive until its wait(); a pinned_array's
        memory goes with the Engine that made it, so it is not handed to another Engine that outlives that one."""
        if not hasattr(self.L, "fpl_process_bgzf_bam_async"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_process_bgzf_bam_async")
        comp = np.ascontiguousarray(comp, dtype=np.uint8)
        blk = np.array(blocks, dtype=np.dtype(abi.BGZF_BLOCK_DTYPE), copy=True, ndmin=1) if len(blocks) else np.zeros(0, np.dtype(abi.BGZF_BLOCK_DTYPE))
        if gzip or self._bam_gz_on:  # (the switch is the context's: touched only when it has to change)
            self._check(self.L.fpl_set_bam_gzip(self.h, int(bool(gzip))), "fpl_set_bam_gzip")
            self._bam_gz_on = bool(gzip)
        self._check(self.L.fpl_process_bgzf_bam_async(self.h, comp.ctypes.data if len(comp) else None, len(comp),
                                                      blk.ctypes.data if len(blk) else None, len(blk), int(skip)), "fpl_process_bgzf_bam_async")
        return BgzfBatch(self, bool(gzip), (comp, blk))

    def submit_bgzf_text(self, comp, blocks, gzip=False):
        """fpl_process_bgzf_text_async: the payloads of a BGZF-compressed FASTQ's blocks and their descriptors, as for submit_bgzf
        (fastplong_amd.bgzf.blocks cuts any BGZF file into them).  Inflate, the cut at a record's end, the parse and the per-read
        kernels all run on the device -> a BgzfTextBatch with peek() and wait().  gzip=True: the passing reads also come back as a
        gzip member.  The tail between two submissions is bam_tail() / set_bam_tail() / resume_bgzf() / reserve_bam_tail()'s."""
        if not hasattr(self.L, "fpl_process_bgzf_text_async"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_process_bgzf_text_async")
        comp = np.ascontiguousarray(comp, dtype=np.uint8)
        blk = np.array(blocks, dtype=np.dtype(abi.BGZF_BLOCK_DTYPE), copy=True, ndmin=1) if len(blocks) else np.zeros(0, np.dtype(abi.BGZF_BLOCK_DTYPE))
        if gzip or getattr(self, "_gz_on", False):  # (the switch is the context's: touched only when it has to change)
            self._check(self.L.fpl_set_text_gzip(self.h, int(bool(gzip))), "fpl_set_text_gzip")
            self._gz_on = bool(gzip)
        self._check(self.L.fpl_process_bgzf_text_async(self.h, comp.ctypes.data if len(comp) else None, len(comp),
                                                       blk.ctypes.data if len(blk) else None, len(blk)), "fpl_process_bgzf_text_async")
        return BgzfTextBatch(self, bool(gzip), (comp, blk))

    def bam_tail(self):
        """fpl_bam_tail_get: the bytes behind the last whole record of the BGZF submissions so far"""
        n = C.c_uint64(0)
        rc = self.L.fpl_bam_tail_get(self.h, None, 0, C.byref(n))
        if rc == abi.FPL_OK or n.value == 0:
            self._check(rc, "fpl_bam_tail_get")
            return b""
        buf = np.zeros(n.value, np.uint8)
        self._check(self.L.fpl_bam_tail_get(self.h, buf.ctypes.data, len(buf), C.byref(n)), "fpl_bam_tail_get")
        return buf[:n.value].tobytes()

    def set_bam_tail(self, data=b""):
        """fpl_bam_tail_set: replaces the tail and clears the refusal flag; b"" starts a new file"""
        buf = np.frombuffer(bytes(data), np.uint8)
        self._check(self.L.fpl_bam_tail_set(self.h, buf.ctypes.data if len(buf) else None, len(buf)), "fpl_bam_tail_set")

    def resume_bgzf(self):
        """fpl_resume_bgzf_bam: clears the refusal flag and keeps the tail"""
        self._check(self.L.fpl_resume_bgzf_bam(self.h), "fpl_resume_bgzf_bam")

    def reserve_bam_tail(self, nbytes):
        self._check(self.L.fpl_reserve_bam_tail(self.h, int(nbytes)), "fpl_reserve_bam_tail")

    def decode_bam(self, bam, rec_start, off):
        """fpl_decode_bam on this engine's device -> (bases, qualities) as uint8 arrays of off[-1] bytes"""
        return decode_bam(self.device, bam, rec_start, off)

    def submit_text(self, text, gzip=False):
        """fpl_process_text_async: a chunk of FASTQ text (a pinned uint8 array: pinned_array) that starts at a record and ends
        behind one; the parse runs on the device"""
        self._keep_text = getattr(self, "_keep_text", []) + [text]
        self._keep_text = self._keep_text[-(abi.FPL_MAX_IN_FLIGHT + 1):]
        if gzip or getattr(self, "_gz_on", False):  # (the switch is the context's: touched only when it has to change)
            if not hasattr(self.L, "fpl_wait_text_gz"):
                raise FplError("gzip=True needs fpl_set_text_gzip / fpl_wait_text_gz (C-ABI version 9)")
            self._check(self.L.fpl_set_text_gzip(self.h, int(bool(gzip))), "fpl_set_text_gzip")
            self._gz_on = bool(gzip)
        self._check(self.L.fpl_process_text_async(self.h, text.ctypes.data, len(text)), "fpl_process_text_async")
        self._gz_flags = getattr(self, "_gz_flags", []) + [bool(gzip)]

    def peek_text(self):
        """fpl_peek_text: the parse's verdict for the oldest text batch (nothing of it is counted yet)"""
        out = abi.FplTextResult()
        self._check(self.L.fpl_peek_text(self.h, C.byref(out)), "fpl_peek_text")
        return {k: getattr(out, k) for k, _ in abi.FplTextResult._fields_}

    def start_text(self):
        """fpl_start_text: the per-read kernels of the next pending text batch"""
        self._check(self.L.fpl_start_text(self.h), "fpl_start_text")

    def cancel_text(self):
        self._check(self.L.fpl_cancel_text(self.h), "fpl_cancel_text")

    def wait_text(self):
        """fpl_wait_text -> (fpl_text_result as a dict, records [n] as a numpy copy, line starts [n, 4] as a numpy copy); for a
        batch submitted with gzip=True fpl_wait_text_gz, and a fourth item: the batch's gzip member as bytes (b"" when no read
        passed)"""
        out = abi.FplTextResult()
        rp, lp = C.c_void_p(), C.c_void_p()
        flags = getattr(self, "_gz_flags", [])
        want_gz = flags.pop(0) if flags else False
        if want_gz:
            gp, gl = C.c_void_p(), C.c_uint64(0)
            self._check(self.L.fpl_wait_text_gz(self.h, C.byref(out), C.byref(rp), C.byref(lp), C.byref(gp), C.byref(gl)), "fpl_wait_text_gz")
            member = (C.string_at(gp.value, gl.value) if gl.value else b"",)
        else:
            self._check(self.L.fpl_wait_text(self.h, C.byref(out), C.byref(rp), C.byref(lp)), "fpl_wait_text")
            member = ()
        info = {k: getattr(out, k) for k, _ in abi.FplTextResult._fields_}
        n = out.n_reads
        if out.status != 0 or n == 0:
            return (info, np.zeros(0, dtype=abi.RESULT_DTYPE), np.zeros((0, 4), np.uint32)) + member
        res = np.ctypeslib.as_array(C.cast(rp, C.POINTER(C.c_uint8)), shape=(n * 36,)).view(abi.RESULT_DTYPE).copy()
        lines = np.ctypeslib.as_array(C.cast(lp, C.POINTER(C.c_uint32)), shape=(n, 4)).copy()
        return (info, res, lines) + member

    def in_flight(self):
        return int(self.L.fpl_in_flight(self.h))

    def pinned_array(self, n, dtype=np.uint8, keep=True):
        """numpy view of n items of page-locked host memory (fpl_host_alloc).  The memory lives as long as this Engine object;
        keep=False: only as long as the array and its views do (the library must be done with it by then)."""
        nbytes = max(1, int(n) * np.dtype(dtype).itemsize)
        ptr = self.L.fpl_host_alloc(nbytes)
        if not ptr:
            raise FplError("fpl_host_alloc(%d) failed" % nbytes)
        L = self.L

        class _Owner:
            def __del__(self_inner):
                L.fpl_host_free(ptr)

        buf = (C.c_uint8 * nbytes).from_address(ptr)
        arr = np.frombuffer(buf, dtype=dtype, count=int(n))
        if keep:
            self._pinned = getattr(self, "_pinned", [])
            self._pinned.append((_Owner(), buf))
        else:
            buf._owner = _Owner()  # (arr and its views hold buf)
        return arr

    def fragments(self):
        """--break / --mask outcome of the LAST batch: (fpl_fragment records sorted by (read, seq_no), fpl_region list)"""
        nf, nr = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.fpl_fragment_counts(self.h, C.byref(nf), C.byref(nr)), "fpl_fragment_counts")
        frags = np.zeros(max(nf.value, 1), dtype=abi.FRAGMENT_DTYPE)
        regs = np.zeros(max(nr.value, 1), dtype=abi.REGION_DTYPE)
        self._check(self.L.fpl_get_fragments(self.h, frags.ctypes.data, nf.value, regs.ctypes.data, nr.value),
                    "fpl_get_fragments")
        return frags[:nf.value], regs[:nr.value]

    def process_device(self, seq_t, qual_t, off_t, max_read_len, results_t=None, stream=None):
        """fpl_process_batch_device on torch CUDA tensors (uint8, uint8, int64 offsets).
        Asynchronous on `stream` (default: torch's current stream)."""
        import torch

        n = off_t.numel() - 1
        if results_t is None:
            results_t = torch.empty(max(n, 1) * C.sizeof(abi.FplReadResult), dtype=torch.uint8, device=seq_t.device)
        if stream is None:
            stream = torch.cuda.current_stream(seq_t.device).cuda_stream
        self._check(self.L.fpl_process_batch_device(self.h, seq_t.data_ptr(), qual_t.data_ptr(), off_t.data_ptr(), n,
                                                    seq_t.numel(), int(max_read_len), results_t.data_ptr(),
                                                    C.c_void_p(stream)), "fpl_process_batch_device")
        return results_t

    def emit_device(self, seq_t, qual_t, off_t, results_t, stream=None, seq_out=None, qual_out=None, off_out=None, src=None, kind=None):
        """fpl_emit_batch_device: the passing, trimmed reads of a batch (the tensors given to process_device and the records it
        wrote) as a CSR batch on the device -> (seq_out, qual_out, off_out, src, kind, info_t).  Tensors that are not given are
        made at the sizes that always suffice (seq_t.numel() bytes, 2 n reads); given ones set the capacities: seq_out and
        qual_out (uint8, equally long), off_out (int64, reads + 1), src (int32) and kind (uint8) with a slot per read off_out
        has room for.  Asynchronous on `stream` (default: torch's current stream) and without a synchronize: the tensors hold
        the batch once the stream has got there, info_t (32 bytes, uint8; emit_info reads it back) says how much of them it
        fills.  Behind a process_device on the same stream the two calls need nothing between them.
        After set_fragment_output(True) on a --break / --mask engine the output reads are the passing fragments of the LAST
        process_device: off_out defaults to the room their number's bound asks for, the bases carry their N, and
        self.emit_break_no (int16, a slot per read off_out has room for) holds break_no of every output read."""
        import torch

        if not hasattr(self.L, "fpl_emit_batch_device"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_emit_batch_device")
        dev = seq_t.device
        n = max(off_t.numel() - 1, 0)
        if seq_out is None:
            seq_out = torch.empty(max(seq_t.numel(), 1), dtype=torch.uint8, device=dev)
        if qual_out is None:
            qual_out = torch.empty(seq_out.numel(), dtype=torch.uint8, device=dev)
        frag_out = getattr(self, "_frag_out", False)
        if off_out is None:
            most = 2 * n
            if frag_out:  # (break_mask_caps, csrc/pipeline.h: every further fragment costs a break window and a base)
                w = int(self.opt.break_window) if self.opt.break_enabled and self.opt.break_window > 0 else 1 << 62
                most = 2 * n + seq_t.numel() // (w + 1) + 16
            off_out = torch.empty(most + 1, dtype=torch.int64, device=dev)
        cap_reads = off_out.numel() - 1
        if frag_out:
            self.emit_break_no = torch.empty(max(cap_reads, 1), dtype=torch.int16, device=dev)
            self._check(self.L.fpl_set_emit_break_no(self.h, self.emit_break_no.data_ptr()), "fpl_set_emit_break_no")
        if src is None:
            src = torch.empty(max(cap_reads, 1), dtype=torch.int32, device=dev)
        if kind is None:
            kind = torch.empty(max(cap_reads, 1), dtype=torch.uint8, device=dev)
        if qual_out.numel() != seq_out.numel() or cap_reads < 0 or src.numel() < cap_reads or kind.numel() < cap_reads:
            raise FplError("emit_device: seq_out / qual_out differ in length, or src / kind are shorter than off_out admits")
        for t, dt in ((seq_out, torch.uint8), (qual_out, torch.uint8), (off_out, torch.int64), (src, torch.int32), (kind, torch.uint8)):
            if t.dtype != dt or not t.is_contiguous() or t.device != dev:
                raise FplError("emit_device: the outputs are contiguous tensors on the batch's device (uint8, uint8, int64, int32, uint8)")
        info_t = torch.empty(32 + 16, dtype=torch.uint8, device=dev)
        spare = info_t[32:].data_ptr()  # (an empty tensor has no address; a capacity of zero bytes is legal and needs one)
        info_t = info_t[:32]
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self.L.fpl_emit_batch_device(self.h, seq_t.data_ptr(), qual_t.data_ptr(), off_t.data_ptr(), n, results_t.data_ptr(),
                                                 seq_out.data_ptr() or spare, qual_out.data_ptr() or spare, seq_out.numel(),
                                                 off_out.data_ptr(), cap_reads, src.data_ptr() or None, kind.data_ptr() or None,
                                                 info_t.data_ptr(), C.c_void_p(stream)),
                    "fpl_emit_batch_device")
        return seq_out, qual_out, off_out, src, kind, info_t

    @staticmethod
    def emit_info(info_t):
        """the 32 bytes of emit_device's info_t, read back (this waits for the stream) -> dict(n_bytes, n_out, max_len, status)"""
        r = info_t.cpu().numpy().view(abi.EMIT_INFO_DTYPE)[0]
        return dict(n_bytes=int(r["n_bytes"]), n_out=int(r["n_out"]), max_len=int(r["max_len"]), status=int(r["status"]))

    @staticmethod
    def results_to_numpy(results_t, n):
        return results_t.cpu().numpy().view(abi.RESULT_DTYPE)[:n]

    def counters(self):
        n = int(self.L.fpl_counters_len(self.h))
        buf = np.zeros(n, dtype=np.int64)
        self._check(self.L.fpl_get_counters(self.h, buf.ctypes.data, n), "fpl_get_counters")
        return buf

    def counters_tensor(self):
        """Zero-copy torch view (int64) of the device counter buffer, e.g. for
        torch.distributed.all_reduce over RCCL.  Invalid after a capacity grow."""
        import torch

        n = int(self.L.fpl_counters_len(self.h))
        ptr = int(self.L.fpl_counters_device_ptr(self.h))

        class _Holder:
            pass

        hld = _Holder()
        hld.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr, False), "version": 2}
        hld._keep = self
        return torch.as_tensor(hld, device="cuda:%d" % self.device)

    def reset_counters(self):
        self._check(self.L.fpl_reset_counters(self.h), "fpl_reset_counters")

    def synchronize(self):
        self._check(self.L.fpl_synchronize(self.h), "fpl_synchronize")

    def enable_timing(self, on=True):
        self._check(self.L.fpl_enable_timing(self.h, int(on)), "fpl_enable_timing")

    def assume_inputs_ready(self, yes=True):
        """the batches handed to process_device are complete on the device when the call is made (resident tensors): the end trims
        of a batch may then start beside the previous batch's kernels (fpl_assume_inputs_ready)"""
        self._check(self.L.fpl_assume_inputs_ready(self.h, int(bool(yes))), "fpl_assume_inputs_ready")

    def batch_forms(self):
        """-> dict: batches, reads, through k_trim_ends_batched, through k_stats_sorted, largest batch, batches whose end trims ran ahead
        (fpl_get_batch_forms)"""
        out = (C.c_uint64 * 6)()
        self._check(self.L.fpl_get_batch_forms(self.h, out), "fpl_get_batch_forms")
        return dict(batches=int(out[0]), reads=int(out[1]), trim_batched=int(out[2]), stats_sorted=int(out[3]), largest=int(out[4]), trims_ahead=int(out[5]))

    def set_gzip_framing(self, bgzf):
        """fpl_set_gzip_framing: the bytes of the gzip batches submitted from now on are BGZF blocks (True; fastplong_amd.bgzf.blocks
        cuts them, bgzf.EOF ends a file of them) or one gzip member per batch (False, the default)"""
        if not hasattr(self.L, "fpl_set_gzip_framing"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_set_gzip_framing")
        self._check(self.L.fpl_set_gzip_framing(self.h, abi.FPL_GZIP_BGZF if bgzf else abi.FPL_GZIP_MEMBER), "fpl_set_gzip_framing")

    def set_fragment_output(self, on):
        """fpl_set_fragment_output: a context with break_enabled / mask_enabled writes its device output forms -- submit_text /
        submit_bam with gzip=True, emit_device -- from the fragment list of its last batch, ordered on the device.  Without
        the two options the call changes nothing."""
        if not hasattr(self.L, "fpl_set_fragment_output"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_set_fragment_output")
        self._check(self.L.fpl_set_fragment_output(self.h, int(bool(on))), "fpl_set_fragment_output")
        self._frag_out = bool(on) and bool(self.opt.break_enabled or self.opt.mask_enabled)

    def set_gzip_records(self, bam):
        """fpl_set_gzip_records: the gzip batches submitted from now on are unaligned BAM records in BGZF blocks (True; a file is
        fastplong_amd.bgzf.bam_header() + the batches' bytes + bgzf.eof()) or FASTQ text (False, the default)"""
        if not hasattr(self.L, "fpl_set_gzip_records"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_set_gzip_records")
        self._check(self.L.fpl_set_gzip_records(self.h, abi.FPL_GZIP_BAM if bam else abi.FPL_GZIP_FASTQ), "fpl_set_gzip_records")

    def set_bam_tags(self, on):
        """fpl_set_bam_tags: the BAM records of the gzip batches submitted from now on (set_gzip_records(True), submit_bam /
        submit_bgzf) carry the auxiliary fields of their input records, by the rule of README "BAM output"; the file's header should
        then repeat the input's @RG lines: fastplong_amd.bgzf.bam_header(read_groups=bgzf.read_group_lines(input header text))"""
        if not hasattr(self.L, "fpl_set_bam_tags"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_set_bam_tags")
        self._check(self.L.fpl_set_bam_tags(self.h, 1 if on else 0), "fpl_set_bam_tags")

    def bam_tag_stats(self):
        """fpl_get_bam_tag_stats -> (records that kept every field, records that lost positional fields, tag bytes written, records
        whose region did not parse to its end), per output record since the engine was made"""
        if not hasattr(self.L, "fpl_get_bam_tag_stats"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_get_bam_tag_stats")
        out = (C.c_uint64 * 4)()
        self._check(self.L.fpl_get_bam_tag_stats(self.h, out), "fpl_get_bam_tag_stats")
        return tuple(int(v) for v in out)

    def set_bam_mods(self, on):
        """fpl_set_bam_mods: with set_bam_tags(True), the trimmed and split records of the batches submitted from now on get their
        MM / ML / MN fields re-indexed for their piece of the read (README "BAM output", --keep_mods) in place of losing them"""
        if not hasattr(self.L, "fpl_set_bam_mods"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_set_bam_mods")
        self._check(self.L.fpl_set_bam_mods(self.h, 1 if on else 0), "fpl_set_bam_mods")

    def bam_mod_stats(self):
        """fpl_get_bam_mod_stats -> (output records re-indexed, changed records whose modification fields were not re-indexable
        and were dropped, modification positions kept, positions cut away), since the engine was made"""
        if not hasattr(self.L, "fpl_get_bam_mod_stats"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_get_bam_mod_stats")
        out = (C.c_uint64 * 4)()
        self._check(self.L.fpl_get_bam_mod_stats(self.h, out), "fpl_get_bam_mod_stats")
        return tuple(int(v) for v in out)

    def set_bam_comments(self, tags):
        """fpl_set_bam_comments: the FASTQ text of the gzip batches submitted from now on (set_bam_gzip(True), submit_bam /
        submit_bgzf, records as FASTQ) carries the auxiliary fields of its reads' input records as comments behind the names, by the
        rule of README "Tags as FASTQ comments".  tags: None or an empty list for off, "*" for every field, or a list of up to 32
        two-character tags (str or bytes)"""
        if not hasattr(self.L, "fpl_set_bam_comments"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_set_bam_comments")
        if tags is None:
            raw, n = b"", 0
        elif isinstance(tags, (str, bytes)) and tags in ("*", b"*"):
            raw, n = b"", -1
        else:
            items = [t.encode() if isinstance(t, str) else bytes(t) for t in tags]
            if any(len(t) != 2 for t in items):
                raise FplError("fpl_set_bam_comments: a tag has two characters")
            raw, n = b"".join(items), len(items)
        self._check(self.L.fpl_set_bam_comments(self.h, raw, n), "fpl_set_bam_comments")

    def bam_comment_stats(self):
        """fpl_get_bam_comment_stats -> (output records that got at least one field, fields written, comment bytes with their tabs,
        fields left out for control bytes), since the engine was made"""
        if not hasattr(self.L, "fpl_get_bam_comment_stats"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_get_bam_comment_stats")
        out = (C.c_uint64 * 4)()
        self._check(self.L.fpl_get_bam_comment_stats(self.h, out), "fpl_get_bam_comment_stats")
        return tuple(int(v) for v in out)

    def set_bam_moves(self, on):
        """fpl_set_bam_moves: with set_bam_tags(True), the trimmed and split records of the batches submitted from now on get their
        move table mv and its ts re-indexed for their piece of the read (README "BAM output", --keep_moves) in place of losing the
        table; independent of set_bam_mods"""
        if not hasattr(self.L, "fpl_set_bam_moves"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_set_bam_moves")
        self._check(self.L.fpl_set_bam_moves(self.h, 1 if on else 0), "fpl_set_bam_moves")

    def bam_move_stats(self):
        """fpl_get_bam_move_stats -> (output records re-indexed, changed records whose move table was not re-indexable and was
        dropped, table entries kept, entries cut away), since the engine was made"""
        if not hasattr(self.L, "fpl_get_bam_move_stats"):
            raise FplError("the loaded libfastplong_amd.so has no fpl_get_bam_move_stats")
        out = (C.c_uint64 * 4)()
        self._check(self.L.fpl_get_bam_move_stats(self.h, out), "fpl_get_bam_move_stats")
        return tuple(int(v) for v in out)

    def gzip_batches(self):
        """batches whose gzip member was made on the device (fpl_get_gzip_batches)"""
        out = C.c_uint64(0)
        self._check(self.L.fpl_get_gzip_batches(self.h, C.byref(out)), "fpl_get_gzip_batches")
        return int(out.value)

    def kernel_times(self):
        """-> ({kernel name: ms summed over the window}, n_batches)"""
        ms = (C.c_float * 16)()
        names = (C.c_char_p * 16)()
        n, nb = C.c_int(0), C.c_int(0)
        self._check(self.L.fpl_get_kernel_times(self.h, ms, names, C.byref(n), C.byref(nb)), "fpl_get_kernel_times")
        return {names[i].decode(): float(ms[i]) for i in range(n.value)}, nb.value
