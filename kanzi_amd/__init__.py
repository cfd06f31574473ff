"""kanzi_amd -- MI355X-native (gfx950 HIP) implementation of Kanzi's per-block hot path.

Python host-side mirror of the reference's plugin interfaces, bound to the C-ABI in
``include/kanzi_hip.h`` with ctypes.  The product path is the HIP library ``libkanzi_hip.so``;
there is NO CPU fallback: importing works everywhere (so the ABI can be inspected), but creating a
:class:`Context` without the library or without a GPU raises.

Reference interfaces mirrored (K/ = java/src/main/java/io/github/flanglet/kanzi/):
  * ``ByteTransform``  K/ByteTransform.java:36,48,56      -> :class:`BWTBlockCodec`, :class:`SBRT`, :class:`ZRLT`
  * ``EntropyEncoder`` K/EntropyEncoder.java:34,41,48     -> :class:`ANSRangeEncoder`, :class:`HuffmanEncoder`, :class:`NullEntropyEncoder`
  * ``EntropyDecoder`` K/EntropyDecoder.java:33           -> :class:`ANSRangeDecoder`, :class:`NullEntropyDecoder`
  * ``Sequence`` / block span of EncodingTask.encodeBlock -> :func:`encode_blocks` / :func:`decode_blocks`
  * ``CompressedOutputStream`` / ``CompressedInputStream`` -> same-named classes (whole .knz stream)
"""
# The decoder keeps four HIP streams busy side by side; HIP shares 4 hardware queues among all streams of a process unless
# GPU_MAX_HW_QUEUES says otherwise WHEN THE RUNTIME STARTS (first HIP call, also PyTorch's).  That is the APPLICATION's setting
# (bench.py and tests/conftest.py export GPU_MAX_HW_QUEUES=8 before importing torch); neither this binding nor the library
# touches the process environment.  Without it the library measures that its streams share queues and falls back to a
# three-stream schedule.
import ctypes
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libkanzi_hip.so")

# transform ids (K/transform/TransformFactory.java:36-60) and entropy ids (K/entropy/EntropyCodecFactory.java)
NONE_TYPE, BWT_TYPE, LZ_TYPE, RLT_TYPE, ZRLT_TYPE, MTFT_TYPE, RANK_TYPE, SRT_TYPE, MM_TYPE, LZX_TYPE, PACK_TYPE, DNA_TYPE = 0, 1, 3, 5, 6, 7, 8, 13, 15, 16, 18, 19
LZP_TYPE = 14
EXE_TYPE = 9
E_NONE, E_HUFFMAN, E_FPAQ, E_RANGE, E_ANS0, E_CM, E_ANS1 = 0, 1, 2, 4, 5, 6, 8
TRANSFORM_IDS = {"NONE": 0, "BWT": 1, "LZ": 3, "RLT": 5, "ZRLT": 6, "MTFT": 7, "RANK": 8, "EXE": 9, "TEXT": 10, "SRT": 13, "LZP": 14, "MM": 15, "LZX": 16, "UTF": 17, "PACK": 18, "DNA": 19}
TEXT_TYPE, UTF_TYPE = 10, 17
# Global.DataType (K/Global.java:40-80), numbered as KZ_DT_* in include/kanzi_hip.h
DATA_TYPES = {"UNDEFINED": 0, "DNA": 1, "SMALL_ALPHABET": 2, "TEXT": 3, "MULTIMEDIA": 4, "EXE": 5, "NUMERIC": 6, "BASE64": 7, "BIN": 8, "UTF8": 9}
ENTROPY_IDS = {"NONE": 0, "HUFFMAN": 1, "FPAQ": 2, "RANGE": 4, "ANS0": 5, "CM": 6, "ANS1": 8}
MEM_HOST, MEM_DEVICE = 0, 1

STAGE_NAMES = ["bwt_fwd", "sbrt_fwd", "zrlt_fwd", "entropy_enc", "frame_enc",
               "entropy_dec", "zrlt_inv", "sbrt_inv", "bwt_inv", "frame_dec", "lz_fwd", "lz_inv", "srt_fwd", "srt_inv", "host_fwd", "host_inv"]


class KanziError(RuntimeError):
    """Mirror of KanziIOException(code) (K/io/KanziIOException.java); code = K/Error.java value."""

    def __init__(self, code, msg=""):
        super().__init__("kanzi error %d %s" % (code, msg))
        self.code = code


class BlockResult(ctypes.Structure):
    _fields_ = [("bits", ctypes.c_int64), ("length", ctypes.c_int32), ("status", ctypes.c_int32),
                ("skipFlags", ctypes.c_uint8), ("mode", ctypes.c_uint8), ("pad", ctypes.c_uint8 * 6)]


_lib = None


def load_library():
    """Load libkanzi_hip.so and declare every symbol of include/kanzi_hip.h. Raises if missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libkanzi_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback for the product path)")
    L = ctypes.CDLL(LIB_PATH)
    c = ctypes
    vp, u8p, i32p, i64p = c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p
    sig = {
        "kz_abi_version": (c.c_int32, []),
        "kz_ctx_create": (vp, [c.c_int32]),
        "kz_ctx_destroy": (None, [vp]),
        "kz_last_error": (c.c_char_p, [vp]),
        "kz_ctx_stream": (vp, [vp]),
        "kz_pin_to_device_numa": (c.c_int32, [c.c_int32]),
        "kz_host_cpus": (c.c_int32, []),
        "kz_host_share": (c.c_int32, [c.c_int32]),
        "kz_ctx_set_checksum": (c.c_int32, [vp, c.c_int32]),
        "kz_ctx_set_skip_blocks": (c.c_int32, [vp, c.c_int32]),
        "kz_ctx_set_block_size": (c.c_int32, [vp, c.c_int32]),
        "kz_ctx_reload_switches": (None, [vp]),
        "kz_host_stage_blocks": (c.c_int64, [c.c_int32, c.c_int32]),
        "kz_ctx_set_entropy": (c.c_int32, [vp, c.c_uint32]),
        "kz_ctx_set_data_type": (c.c_int32, [vp, c.c_int32]),
        "kz_ctx_get_data_type": (c.c_int32, [vp]),
        "kz_ctx_reset": (c.c_int32, [vp]),
        "kz_transform_forward": (c.c_int32, [vp, c.c_uint32, u8p, c.c_int32, u8p, c.c_int32, i32p]),
        "kz_transform_inverse": (c.c_int32, [vp, c.c_uint32, u8p, c.c_int32, u8p, c.c_int32, i32p]),
        "kz_transform_max_encoded_len": (c.c_int32, [c.c_uint32, c.c_int32]),
        "kz_host_stage_forward": (c.c_int32, [c.c_uint32, c.c_uint32, c.c_int32, i32p, u8p, c.c_int32, u8p, c.c_int32, i32p]),
        "kz_host_stage_inverse": (c.c_int32, [c.c_uint32, c.c_int32, u8p, c.c_int32, u8p, c.c_int32, i32p]),
        "kz_entropy_encode": (c.c_int64, [vp, c.c_uint32, u8p, c.c_int32, u8p, c.c_int64]),
        "kz_entropy_decode": (c.c_int32, [vp, c.c_uint32, u8p, c.c_int64, u8p, c.c_int32, i64p]),
        "kz_encode_blocks": (c.c_int32, [vp, c.c_uint64, c.c_uint32, u8p, c.c_int64, i32p, c.c_int32, u8p, c.c_int64, vp, c.c_int32]),
        "kz_decode_blocks": (c.c_int32, [vp, c.c_uint64, c.c_uint32, c.c_int32, u8p, c.c_int64, i64p, c.c_int32, u8p, c.c_int64, vp, c.c_int32]),
        "kz_max_block_stream_bytes": (c.c_int64, [c.c_int32]),
        "kz_submit_encode_blocks": (c.c_int64, [vp, c.c_uint64, c.c_uint32, u8p, c.c_int64, i32p, c.c_int32, u8p, c.c_int64, vp, c.c_int32]),
        "kz_submit_decode_blocks": (c.c_int64, [vp, c.c_uint64, c.c_uint32, c.c_int32, u8p, c.c_int64, i64p, c.c_int32, u8p, c.c_int64, vp, c.c_int32]),
        "kz_wait": (c.c_int32, [vp, c.c_int64]),
        "kz_poll": (c.c_int32, [vp, c.c_int64]),
        "kz_compress": (c.c_int64, [vp, c.c_uint64, c.c_uint32, c.c_int32, u8p, c.c_int64, u8p, c.c_int64]),
        "kz_decompress": (c.c_int64, [vp, u8p, c.c_int64, u8p, c.c_int64]),
        "kz_compress_bound": (c.c_int64, [c.c_int64, c.c_int32]),
        "kz_transform_type": (c.c_uint64, [i32p, c.c_int32]),
        "kz_knz_assemble": (c.c_int64, [c.c_uint64, c.c_uint32, c.c_int32, c.c_int64, c.c_int32, u8p, c.c_int64, i64p, c.c_int32, u8p, c.c_int64]),
        "kz_knz_writer_open": (vp, [c.c_uint64, c.c_uint32, c.c_int32, c.c_int64, c.c_int32, u8p, c.c_int64]),
        "kz_knz_writer_add": (c.c_int32, [vp, u8p, c.c_int64]),
        "kz_knz_writer_close": (c.c_int64, [vp]),
        "kz_knz_index": (c.c_int32, [u8p, c.c_int64, vp, vp, vp, vp, vp, i64p, i64p, c.c_int32]),
        "kz_knz_scan": (c.c_int64, [u8p, c.c_int64, c.c_int32, vp, vp, vp, vp, vp, i64p, i64p, i64p, i64p, c.c_int64, i64p]),
        "kz_knz_scan_device": (c.c_int64, [vp, u8p, c.c_int64, c.c_int32, vp, vp, vp, vp, vp, i64p, i64p, i64p, i64p, c.c_int64, i64p]),
        "kz_compress_device": (c.c_int64, [vp, c.c_uint64, c.c_uint32, c.c_int32, u8p, c.c_int64, u8p, c.c_int64]),
        "kz_decompress_device": (c.c_int64, [vp, u8p, c.c_int64, u8p, c.c_int64]),
        "kz_knz_assemble_device": (c.c_int64, [vp, c.c_uint64, c.c_uint32, c.c_int32, c.c_int64, c.c_int32, u8p, c.c_int64, i64p, c.c_int32, u8p, c.c_int64]),
        "kz_knz_index_device": (c.c_int32, [vp, u8p, c.c_int64, vp, vp, vp, vp, vp, i64p, i64p, c.c_int32]),
        "kz_compress_many_bound": (c.c_int64, [i64p, c.c_int32, c.c_int32]),
        "kz_compress_many_device": (c.c_int32, [vp, c.c_uint64, c.c_uint32, c.c_int32, u8p, i64p, i64p, c.c_int32, u8p, i64p, i64p, i64p]),
        "kz_decompress_many_device": (c.c_int32, [vp, u8p, i64p, i64p, c.c_int32, u8p, i64p, i64p, i64p]),
        "kz_decompress_range": (c.c_int64, [vp, u8p, c.c_int64, c.c_int64, c.c_int64, u8p, c.c_int64]),
        "kz_decompress_range_device": (c.c_int64, [vp, u8p, c.c_int64, c.c_int64, c.c_int64, u8p, c.c_int64]),
        "kz_decode_indexed": (c.c_int32, [vp, u8p, c.c_int64, i64p, i64p, c.c_int32, u8p, c.c_int64, vp]),
        "kz_decode_indexed_device": (c.c_int32, [vp, u8p, c.c_int64, i64p, i64p, c.c_int32, u8p, c.c_int64, vp]),
        "kz_read_bytes": (c.c_int64, [vp, u8p, c.c_int64, i64p, i64p, i64p, c.c_int32, i64p, i64p, c.c_int32, u8p, c.c_int64, i64p]),
        "kz_read_bytes_device": (c.c_int64, [vp, u8p, c.c_int64, i64p, i64p, i64p, c.c_int32, i64p, i64p, c.c_int32, u8p, c.c_int64, i64p]),
        "kz_knz_index_many_device": (c.c_int64, [vp, u8p, i64p, i64p, c.c_int32, vp, vp, vp, vp, vp, i32p, i64p, i64p, i64p, c.c_int64]),
        "kz_read_bytes_many_device": (c.c_int64, [vp, u8p, i64p, i64p, c.c_int32, i64p, i64p, i64p, i64p, i64p, i32p, i64p, i64p, c.c_int32, u8p, c.c_int64, i64p, i32p]),
        "kz_write_bytes_bound": (c.c_int64, [i64p, c.c_int32, c.c_int32]),
        "kz_write_bytes": (c.c_int64, [vp, u8p, c.c_int64, i64p, i64p, i64p, c.c_int32, i64p, i64p, c.c_int32, u8p, c.c_int64, u8p, c.c_int64, i64p, i64p]),
        "kz_write_bytes_device": (c.c_int64, [vp, u8p, c.c_int64, i64p, i64p, i64p, c.c_int32, i64p, i64p, c.c_int32, u8p, c.c_int64, u8p, c.c_int64, i64p, i64p]),
        "kz_write_bytes_many_bound": (c.c_int64, [i64p, i64p, i32p, c.c_int32, i64p]),
        "kz_write_bytes_many_device": (c.c_int32, [vp, u8p, i64p, i64p, c.c_int32, i64p, i64p, i64p, i64p, i64p, i32p, i64p, i64p, c.c_int32, u8p, c.c_int64,
                                                   u8p, i64p, i64p, i64p, i64p, i64p]),
        "kz_knz_splice_bound": (c.c_int64, [i64p, c.c_int32]),
        "kz_knz_splice": (c.c_int64, [u8p, i64p, i64p, c.c_int32, i32p, i64p, i64p, c.c_int32, c.c_int64, u8p, c.c_int64]),
        "kz_knz_splice_device": (c.c_int64, [vp, u8p, i64p, i64p, c.c_int32, i32p, i64p, i64p, c.c_int32, c.c_int64, u8p, c.c_int64]),
        "kz_set_timing": (None, [vp, c.c_int32]),
        "kz_get_stage_count": (c.c_int32, [vp]),
        "kz_get_stage_ms": (c.c_float, [vp, c.c_int32]),
        "kz_get_stage_alg_bytes": (c.c_int64, [vp, c.c_int32]),
        "kz_reset_timing": (None, [vp]),
        "kz_set_kernel_timing": (None, [vp, c.c_int32]),
        "kz_get_kernel_count": (c.c_int32, []),
        "kz_get_kernel_name": (c.c_char_p, [c.c_int32]),
        "kz_get_kernel_ms": (c.c_double, [vp, c.c_int32]),
        "kz_get_kernel_max_ms": (c.c_double, [vp, c.c_int32]),
        "kz_get_kernel_launches": (c.c_int64, [vp, c.c_int32]),
        "kz_reset_kernel_timing": (None, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)          # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


ABI_SYMBOLS = ["kz_abi_version", "kz_ctx_create", "kz_ctx_destroy", "kz_last_error", "kz_ctx_stream", "kz_pin_to_device_numa", "kz_host_cpus", "kz_host_share", "kz_ctx_set_checksum",
               "kz_ctx_set_data_type", "kz_ctx_get_data_type", "kz_ctx_reset", "kz_ctx_set_skip_blocks", "kz_ctx_set_block_size", "kz_ctx_reload_switches", "kz_host_stage_blocks", "kz_ctx_set_entropy",
               "kz_transform_forward", "kz_transform_inverse", "kz_transform_max_encoded_len", "kz_host_stage_forward", "kz_host_stage_inverse",
               "kz_entropy_encode", "kz_entropy_decode", "kz_encode_blocks", "kz_decode_blocks",
               "kz_max_block_stream_bytes", "kz_submit_encode_blocks", "kz_submit_decode_blocks", "kz_wait", "kz_poll", "kz_compress", "kz_decompress", "kz_compress_bound", "kz_transform_type",
               "kz_knz_assemble", "kz_knz_index", "kz_knz_writer_open", "kz_knz_writer_add", "kz_knz_writer_close",
               "kz_compress_device", "kz_decompress_device", "kz_knz_assemble_device", "kz_knz_index_device",
               "kz_compress_many_bound", "kz_compress_many_device", "kz_decompress_many_device",
               "kz_decompress_range", "kz_decompress_range_device", "kz_decode_indexed", "kz_decode_indexed_device",
               "kz_read_bytes", "kz_read_bytes_device", "kz_knz_index_many_device", "kz_read_bytes_many_device",
               "kz_write_bytes_bound", "kz_write_bytes", "kz_write_bytes_device", "kz_write_bytes_many_bound", "kz_write_bytes_many_device",
               "kz_knz_splice_bound", "kz_knz_splice", "kz_knz_splice_device",
               "kz_knz_scan", "kz_knz_scan_device",
               "kz_set_timing", "kz_get_stage_count", "kz_get_stage_ms", "kz_get_stage_alg_bytes", "kz_reset_timing",
               "kz_set_kernel_timing", "kz_get_kernel_count", "kz_get_kernel_name", "kz_get_kernel_ms", "kz_get_kernel_max_ms",
               "kz_get_kernel_launches", "kz_reset_kernel_timing"]


# The reference's compression levels (K/app/BlockCompressor.java:537-573, getTransformAndCodec) as "transforms&entropy".
# Levels 0-3, 5 and 6 consist of stages built here (TEXT and UTF run as host stages in front of the GPU chain);
# 4, 8 and 9 need ROLZ / TPAQ.  Every stage of level 7 is built (LZP, CM), but it puts LZP in front of TEXT and UTF, and the host
# stages only run in front of the GPU stages: level_chain refuses that order, as it refuses levels 8 and 9 for EXE + RLT there.
LEVELS = {0: "NONE&NONE", 1: "LZX&NONE", 2: "DNA+LZ&HUFFMAN", 3: "TEXT+UTF+PACK+MM+LZX&HUFFMAN", 4: "TEXT+UTF+EXE+PACK+MM+ROLZ&NONE",
          5: "TEXT+UTF+BWT+RANK+ZRLT&ANS0", 6: "TEXT+UTF+BWT+SRT+ZRLT&FPAQ", 7: "LZP+TEXT+UTF+BWT+LZP&CM",
          8: "EXE+RLT+TEXT+UTF+DNA&TPAQ", 9: "EXE+RLT+TEXT+UTF+DNA&TPAQX"}


def level_chain(level, allow_partial=False):
    """(transform string, entropy name) of a reference level.  Raises for a level with stages that are not built, unless
    allow_partial drops the leading TEXT+UTF pair (the result is then NOT level-exact on blocks those stages accept)."""
    t, e = LEVELS[int(level)].split("&")
    names = t.split("+")
    if allow_partial and names[:2] == ["TEXT", "UTF"]:
        names = names[2:]
    missing = [n for n in names if n not in TRANSFORM_IDS] + ([e] if e not in ENTROPY_IDS else [])
    if missing:
        raise KanziError(3, "level %d needs %s, not built here" % (level, "/".join(missing)))       # ERR_INVALID_CODEC
    host = [n in ("TEXT", "UTF") for n in names]
    if any(host[i] and not host[i - 1] for i in range(1, len(names))):
        raise KanziError(3, "level %d puts %s in front of TEXT / UTF: the host stages run only in front of the GPU stages (stage order)"
                         % (level, "+".join(names[:host.index(True)])))
    return "+".join(names), e


def host_stage_forward(name, data, entropy="NONE", block_size=4 * 1024 * 1024, data_type=0, cap=None):
    """TEXT / UTF forward on the host (no context, no GPU) -> (applied, bytes, data type after the call)"""
    L = load_library()
    a = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
    t = TRANSFORM_IDS[name.upper()]
    if cap is None:
        cap = int(L.kz_transform_max_encoded_len(t, len(a)))
    out = np.zeros(max(cap, 1) + 64, dtype=np.uint8)
    p, dt = ctypes.c_int32(0), ctypes.c_int32(int(data_type))
    r = L.kz_host_stage_forward(t, ENTROPY_IDS[entropy.upper()], int(block_size), ctypes.addressof(dt), a.ctypes.data if len(a) else out.ctypes.data, len(a),
                                out.ctypes.data, cap, ctypes.addressof(p))
    if r < 0:
        raise KanziError(-r, "host_stage_forward")
    return bool(r), out[:p.value].tobytes(), int(dt.value)


def host_stage_inverse(name, data, cap, block_size=4 * 1024 * 1024):
    """TEXT / UTF inverse on the host -> (ok, bytes)"""
    L = load_library()
    a = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
    out = np.zeros(max(cap, 1) + 64, dtype=np.uint8)
    p = ctypes.c_int32(0)
    r = L.kz_host_stage_inverse(TRANSFORM_IDS[name.upper()], int(block_size), a.ctypes.data if len(a) else out.ctypes.data, len(a), out.ctypes.data, cap, ctypes.addressof(p))
    if r < 0:
        raise KanziError(-r, "host_stage_inverse")
    return bool(r), out[:p.value].tobytes()


def transform_type(names):
    """'BWT+RANK+ZRLT' or a list of names/ids -> 48-bit id word (TransformFactory.java:132-158)."""
    if isinstance(names, str):
        names = [s for s in names.split("+") if s]
    ids = [TRANSFORM_IDS[x.upper()] if isinstance(x, str) else int(x) for x in names]
    if not 1 <= len(ids) <= 8:
        raise ValueError("Only 1 to 8 transforms allowed")          # Sequence.java:42-43
    t = 0
    for i in range(8):
        t = (t << 6) | (ids[i] if i < len(ids) else 0)
    return t


def _ptr(a):
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a)


_LIVE = weakref.WeakSet()


def reload_switches():
    """every live Context reads the KZ_* environment switches again (they are read once, at creation)"""
    for c in list(_LIVE):
        c.reload_switches()


class Context:
    """One HIP stream + scratch arena on one GPU (kz_ctx). Not thread-safe, like a reference codec instance."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.h = self.lib.kz_ctx_create(int(device))
        if not self.h:
            raise RuntimeError("kz_ctx_create(%d) failed: no usable HIP device (the HIP path has no CPU fallback)" % device)
        _LIVE.add(self)

    def close(self):
        if getattr(self, "h", None):
            self.lib.kz_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reload_switches(self):
        """The KZ_* environment switches are read once, when the context is created: read them again (tests, A/B tools)."""
        if getattr(self, "h", None):
            self.lib.kz_ctx_reload_switches(self.h)

    def error(self):
        return self.lib.kz_last_error(self.h).decode("utf-8", "replace")

    def check(self, rc):
        if rc < 0:
            raise KanziError(-rc, self.error())
        return rc

    def set_checksum(self, bits):
        """0, 32 or 64: block checksum kind (the reference's -x32 / -x64)."""
        self.check(self.lib.kz_ctx_set_checksum(self.h, int(bits)))

    def set_skip_blocks(self, on):
        """The context map's "skipBlocks" entry (CLI --skip): incompressible-looking blocks become copy blocks."""
        self.check(self.lib.kz_ctx_set_skip_blocks(self.h, 1 if on else 0))

    def set_block_size(self, block_size):
        """The context map's "blockSize" entry (the stream's block size): TEXT sizes its hash map by it."""
        self.check(self.lib.kz_ctx_set_block_size(self.h, int(block_size)))

    def set_entropy(self, entropy):
        """The context map's "entropy" entry for single-transform calls: TEXT is TextCodec2 for NONE/ANS0/HUFFMAN/RANGE, else TextCodec1."""
        self.check(self.lib.kz_ctx_set_entropy(self.h, ENTROPY_IDS[entropy.upper()] if isinstance(entropy, str) else int(entropy)))

    def set_data_type(self, data_type):
        """The context map's "dataType" entry (a DATA_TYPES name or value) that the next transform instance will see."""
        dt = DATA_TYPES[data_type.upper()] if isinstance(data_type, str) else int(data_type)
        self.check(self.lib.kz_ctx_set_data_type(self.h, dt))

    def reset(self):
        """Every set_* value back to a fresh context's."""
        self.check(self.lib.kz_ctx_reset(self.h))

    def get_data_type(self):
        """What the last forward transform left in the context's "dataType" entry (DATA_TYPES value)."""
        return int(self.lib.kz_ctx_get_data_type(self.h))

    @property
    def stream(self):
        return self.lib.kz_ctx_stream(self.h)

    # ---- instrumentation ----
    def set_timing(self, on):
        self.lib.kz_set_timing(self.h, 1 if on else 0)

    def reset_timing(self):
        self.lib.kz_reset_timing(self.h)

    def set_kernel_timing(self, on):
        self.lib.kz_set_kernel_timing(self.h, 1 if on else 0)

    def reset_kernel_timing(self):
        self.lib.kz_reset_kernel_timing(self.h)

    def kernel_times(self):
        """{kernel name: {"ms": summed launch durations, "launches": n, "max_ms": longest launch}} since the last reset."""
        out = {}
        for i in range(self.lib.kz_get_kernel_count()):
            n = int(self.lib.kz_get_kernel_launches(self.h, i))
            if n:
                out[self.lib.kz_get_kernel_name(i).decode()] = {"ms": float(self.lib.kz_get_kernel_ms(self.h, i)), "launches": n,
                                                                "max_ms": float(self.lib.kz_get_kernel_max_ms(self.h, i))}
        return out

    def stage_times(self):
        out = {}
        for i, nm in enumerate(STAGE_NAMES):
            ms = float(self.lib.kz_get_stage_ms(self.h, i))
            if ms > 0:
                out[nm] = {"ms": ms, "alg_bytes": int(self.lib.kz_get_stage_alg_bytes(self.h, i))}
        return out


class SliceByteArray:
    """K/SliceByteArray.java:35-37."""

    def __init__(self, array=None, length=None, index=0):
        self.array = array if array is not None else np.zeros(0, dtype=np.uint8)
        self.length = len(self.array) if length is None else length
        self.index = index


class _Transform:
    """ByteTransform mirror. forward/inverse return True (applied) or False (declined), advancing
    src.index / dst.index exactly like the reference codecs do on success."""
    TYPE = None

    def __init__(self, ctx):
        self.ctx = ctx

    def getMaxEncodedLength(self, n):
        return int(self.ctx.lib.kz_transform_max_encoded_len(self.TYPE, n))

    def _run(self, fn, src, dst, cap=None):
        if src.length == 0:
            return True
        s = np.ascontiguousarray(src.array[src.index:src.index + src.length], dtype=np.uint8)
        if cap is None:
            cap = len(dst.array) - dst.index if fn is self.ctx.lib.kz_transform_inverse else dst.length - dst.index
        if cap <= 0:
            return False
        out = np.empty(cap, dtype=np.uint8)
        produced = ctypes.c_int32(0)
        rc = fn(self.ctx.h, self.TYPE, s.ctypes.data, src.length, out.ctypes.data, cap, ctypes.addressof(produced))
        self.ctx.check(rc)
        if rc == 0:
            return False
        dst.array[dst.index:dst.index + produced.value] = out[:produced.value]
        src.index += src.length
        dst.index += produced.value
        return True

    def forward(self, src, dst):
        return self._run(self.ctx.lib.kz_transform_forward, src, dst)

    def inverse(self, src, dst):
        return self._run(self.ctx.lib.kz_transform_inverse, src, dst)


class BWTBlockCodec(_Transform):
    TYPE = BWT_TYPE            # K/transform/BWTBlockCodec.java


class TextCodec(_Transform):
    """K/transform/TextCodec.java (host stage).  Like the reference's constructor it takes the variant from the context map:
    entropy (TextCodec2 for NONE / ANS0 / HUFFMAN / RANGE, else TextCodec1) and blockSize (hash map size).  In batched encodes the
    forward of either codec runs on the device for large batches (KZ_TEXT_FWD_GPU / KZ_TEXT1_FWD_GPU)."""
    TYPE = TEXT_TYPE

    def __init__(self, ctx, entropy="NONE", blockSize=4 * 1024 * 1024):
        super().__init__(ctx)
        ctx.set_entropy(entropy)
        ctx.set_block_size(blockSize)


class UTFCodec(_Transform):
    TYPE = UTF_TYPE            # K/transform/UTFCodec.java (host stage)


class ZRLT(_Transform):
    TYPE = ZRLT_TYPE           # K/transform/ZRLT.java


class RLT(_Transform):
    """K/transform/RLT.java.  Like the reference's constructor with a context map it reads the entropy coder (the escape symbol is
    searched, and the block's data type looked at, under every coder but NONE / ANS0 / HUFFMAN / RANGE) and the context's
    "dataType" entry (``ctx.set_data_type``), which it may rewrite.  Its forward bounds the output by the length of the output ARRAY
    (RLT.java:115), so the whole array behind ``dst.index`` is handed down, not the slice."""
    TYPE = RLT_TYPE

    def __init__(self, ctx, entropy="NONE"):
        super().__init__(ctx)
        ctx.set_entropy(entropy)

    def forward(self, src, dst):
        if dst.length - dst.index < self.getMaxEncodedLength(src.length):      # RLT.java:86-87
            return False
        return self._run(self.ctx.lib.kz_transform_forward, src, dst, cap=len(dst.array) - dst.index)


class SRT(_Transform):
    TYPE = SRT_TYPE            # K/transform/SRT.java


class FSDCodec(_Transform):
    TYPE = MM_TYPE             # K/transform/FSDCodec.java (transform name "MM")


class AliasCodec(_Transform):
    """K/transform/AliasCodec.java: transform "PACK"; onlyDNA=True is transform "DNA" (TransformFactory.java:341-343)."""

    def __init__(self, ctx, onlyDNA=False):
        super().__init__(ctx)
        self.TYPE = DNA_TYPE if onlyDNA else PACK_TYPE


class LZCodec(_Transform):
    """K/transform/LZCodec.java (LZXCodec): lz=LZ_TYPE or LZX_TYPE."""

    def __init__(self, ctx, lz=LZ_TYPE):
        super().__init__(ctx)
        self.TYPE = lz


class LZPCodec(_Transform):
    TYPE = LZP_TYPE            # K/transform/LZCodec.java:973-1287 (LZPCodec), bitstream 7: minMatch 64


class EXECodec(_Transform):
    """K/transform/EXECodec.java, bitstream >= 3.  Its forward reads the context's "dataType" entry (``ctx.set_data_type``: only
    UNDEFINED, EXE and BIN blocks are looked at) and writes EXE when it applies."""
    TYPE = EXE_TYPE


class SBRT(_Transform):
    MODE_MTF, MODE_RANK, MODE_TIMESTAMP = 1, 2, 3   # K/transform/SBRT.java:35-37

    def __init__(self, ctx, mode=2):
        super().__init__(ctx)
        if mode not in (1, 2):
            raise ValueError("Invalid mode parameter")
        self.TYPE = RANK_TYPE if mode == 2 else MTFT_TYPE


class _EntropyEncoder:
    TYPE = None

    def __init__(self, ctx):
        self.ctx = ctx
        self.bits = []         # list of (bytes, nbits) appended, like the OutputBitStream given at construction

    def encode(self, block, blkptr, count):
        """EntropyEncoder.encode: returns count on success. Output bit string appended to self.bits."""
        s = np.ascontiguousarray(block[blkptr:blkptr + count], dtype=np.uint8) if count else np.zeros(1, dtype=np.uint8)
        cap = int(self.ctx.lib.kz_max_block_stream_bytes(count))
        if self.TYPE == E_ANS1:
            cap += 102400 * (count // (1 << 22) + 1)            # up to 256 context headers per 4 MiB chunk (include/kanzi_hip.h)
        if self.TYPE == E_RANGE:
            cap = max(cap, (count // (1 << 15) + 1) * (512 + 51200) + 1024)   # the encoder's payload bound per 32 KiB chunk (include/kanzi_hip.h)
        out = np.zeros(cap, dtype=np.uint8)
        nbits = self.ctx.lib.kz_entropy_encode(self.ctx.h, self.TYPE, s.ctypes.data, count, out.ctypes.data, cap)
        self.ctx.check(nbits)
        self.bits.append((out[:(nbits + 7) // 8].tobytes(), int(nbits)))
        return count

    def dispose(self):
        pass


class _EntropyDecoder:
    TYPE = None

    def __init__(self, ctx, data, nbits):
        self.ctx, self.data, self.nbits = ctx, data, nbits

    def decode(self, block, blkptr, count):
        if count == 0:
            return 0
        s = np.frombuffer(bytes(self.data) + b"\0" * 16, dtype=np.uint8)
        out = np.empty(count, dtype=np.uint8)
        used = ctypes.c_int64(0)
        rc = self.ctx.lib.kz_entropy_decode(self.ctx.h, self.TYPE, s.ctypes.data, self.nbits, out.ctypes.data, count, ctypes.addressof(used))
        if rc < 0:
            return -1
        self.bits_consumed = used.value          # the Java adapter advances the shared InputBitStream by this many bits
        block[blkptr:blkptr + count] = out
        return count


class ANSRangeEncoder(_EntropyEncoder):
    """K/entropy/ANSRangeEncoder.java as EntropyCodecFactory builds it: order 0 is ANS0, order 1 is ANS1 (:175-179)."""
    TYPE = E_ANS0

    def __init__(self, ctx, order=0):
        if order not in (0, 1):
            raise ValueError("ANS Codec: The order must be 0 or 1")
        super().__init__(ctx)
        self.TYPE = E_ANS1 if order == 1 else E_ANS0


class ANSRangeDecoder(_EntropyDecoder):
    """K/entropy/ANSRangeDecoder.java: order 0 is ANS0, order 1 is ANS1 (EntropyCodecFactory.java:124-128)."""
    TYPE = E_ANS0

    def __init__(self, ctx, data, nbits, order=0):
        if order not in (0, 1):
            raise ValueError("ANS Codec: The order must be 0 or 1")
        super().__init__(ctx, data, nbits)
        self.TYPE = E_ANS1 if order == 1 else E_ANS0


class HuffmanEncoder(_EntropyEncoder):
    TYPE = E_HUFFMAN           # K/entropy/HuffmanEncoder.java


class HuffmanDecoder(_EntropyDecoder):
    TYPE = E_HUFFMAN


class FPAQEncoder(_EntropyEncoder):
    TYPE = E_FPAQ              # K/entropy/FPAQEncoder.java (encode + dispose)


class FPAQDecoder(_EntropyDecoder):
    TYPE = E_FPAQ


class RangeEncoder(_EntropyEncoder):
    TYPE = E_RANGE             # K/entropy/RangeEncoder.java as EntropyCodecFactory builds it (32 KiB chunks, logRange 12)


class RangeDecoder(_EntropyDecoder):
    TYPE = E_RANGE             # K/entropy/RangeDecoder.java


class CMEncoder(_EntropyEncoder):
    TYPE = E_CM                # K/entropy/BinaryEntropyEncoder.java over K/entropy/CMPredictor.java (encode + dispose); blocks below 1 << 26 bytes


class CMDecoder(_EntropyDecoder):
    TYPE = E_CM                # K/entropy/BinaryEntropyDecoder.java over K/entropy/CMPredictor.java


class NullEntropyEncoder(_EntropyEncoder):
    TYPE = E_NONE


class NullEntropyDecoder(_EntropyDecoder):
    TYPE = E_NONE


def max_block_stream_bytes(n):
    return int(load_library().kz_max_block_stream_bytes(int(n)))


def encode_blocks(ctx, transform, entropy, inp, in_stride, lengths, out, out_stride, mem=MEM_HOST):
    """Fused batched encode (kz_encode_blocks). `inp`/`out`: numpy uint8 arrays (host) or integer device
    pointers (mem=MEM_DEVICE). Returns a ctypes array of BlockResult."""
    tt = transform if isinstance(transform, int) else transform_type(transform)
    et = entropy if isinstance(entropy, int) else ENTROPY_IDS[entropy.upper()]
    lens = np.ascontiguousarray(lengths, dtype=np.int32)
    res = (BlockResult * len(lens))()
    rc = ctx.lib.kz_encode_blocks(ctx.h, tt, et, _ptr(inp), int(in_stride), lens.ctypes.data, len(lens),
                                  _ptr(out), int(out_stride), ctypes.addressof(res), mem)
    ctx.check(rc)
    return res


def decode_blocks(ctx, transform, entropy, block_size, inp, in_stride, bit_lengths, out, out_stride, mem=MEM_HOST):
    tt = transform if isinstance(transform, int) else transform_type(transform)
    et = entropy if isinstance(entropy, int) else ENTROPY_IDS[entropy.upper()]
    bl = np.ascontiguousarray(bit_lengths, dtype=np.int64)
    res = (BlockResult * len(bl))()
    rc = ctx.lib.kz_decode_blocks(ctx.h, tt, et, int(block_size), _ptr(inp), int(in_stride), bl.ctypes.data, len(bl),
                                  _ptr(out), int(out_stride), ctypes.addressof(res), mem)
    ctx.check(rc)
    return res


class Job:
    """A batch queued with submit_encode_blocks / submit_decode_blocks; wait() -> the BlockResult array.  Keeps the arrays the
    C side still points at alive."""

    def __init__(self, ctx, job, res, keep):
        self.ctx, self.job, self.res, self._keep = ctx, job, res, keep

    def done(self):
        return bool(self.ctx.lib.kz_poll(self.ctx.h, self.job))

    def wait(self):
        self.ctx.check(self.ctx.lib.kz_wait(self.ctx.h, self.job))
        return self.res


def submit_encode_blocks(ctx, transform, entropy, inp, in_stride, lengths, out, out_stride, mem=MEM_HOST):
    """kz_submit_encode_blocks: returns a Job at once; the call runs on the context's worker thread."""
    tt = transform if isinstance(transform, int) else transform_type(transform)
    et = entropy if isinstance(entropy, int) else ENTROPY_IDS[entropy.upper()]
    lens = np.ascontiguousarray(lengths, dtype=np.int32)
    res = (BlockResult * len(lens))()
    job = ctx.lib.kz_submit_encode_blocks(ctx.h, tt, et, _ptr(inp), int(in_stride), lens.ctypes.data, len(lens),
                                          _ptr(out), int(out_stride), ctypes.addressof(res), mem)
    ctx.check(min(job, 0))
    return Job(ctx, job, res, (lens, inp, out))


def submit_decode_blocks(ctx, transform, entropy, block_size, inp, in_stride, bit_lengths, out, out_stride, mem=MEM_HOST):
    tt = transform if isinstance(transform, int) else transform_type(transform)
    et = entropy if isinstance(entropy, int) else ENTROPY_IDS[entropy.upper()]
    bl = np.ascontiguousarray(bit_lengths, dtype=np.int64)
    res = (BlockResult * len(bl))()
    job = ctx.lib.kz_submit_decode_blocks(ctx.h, tt, et, int(block_size), _ptr(inp), int(in_stride), bl.ctypes.data, len(bl),
                                          _ptr(out), int(out_stride), ctypes.addressof(res), mem)
    ctx.check(min(job, 0))
    return Job(ctx, job, res, (bl, inp, out))


class CompressedOutputStream:
    """K/io/CompressedOutputStream.java: write() bytes, close() -> .knz bytes in self.output.
    ctx keys mirror the reference's Map (transform, entropy, blockSize)."""

    def __init__(self, ctx, transform="BWT+RANK+ZRLT", entropy="ANS0", blockSize=4 * 1024 * 1024, checksum=0, skipBlocks=False):
        if blockSize > 1024 * 1024 * 1024:
            raise ValueError("The block size must be at most 1 GB")              # CompressedOutputStream.java:165-174
        if blockSize < 1024:
            raise ValueError("The block size must be at least 1024")
        if blockSize & 15:
            raise ValueError("The block size must be a multiple of 16")
        self.ctx = ctx
        self.tt = transform_type(transform)
        self.et = ENTROPY_IDS[entropy.upper()]
        self.blockSize = blockSize
        self.checksum = checksum
        self.skipBlocks = skipBlocks
        self._chunks = []
        self.closed = False
        self.output = None

    def write(self, data):
        if self.closed:
            raise KanziError(12, "Stream closed")                                # ERR_WRITE_FILE
        self._chunks.append(bytes(data))

    def close(self):
        if self.closed:
            return
        self.closed = True
        src = np.frombuffer(b"".join(self._chunks), dtype=np.uint8)
        n = len(src)
        cap = int(self.ctx.lib.kz_compress_bound(n, self.blockSize))
        dst = np.empty(cap, dtype=np.uint8)
        sp = src.ctypes.data if n else dst.ctypes.data
        self.ctx.set_checksum(self.checksum)
        self.ctx.set_skip_blocks(self.skipBlocks)
        try:
            rc = self.ctx.lib.kz_compress(self.ctx.h, self.tt, self.et, self.blockSize, sp, n, dst.ctypes.data, cap)
        finally:
            self.ctx.set_checksum(0)
            self.ctx.set_skip_blocks(False)
        self.ctx.check(rc)
        self.output = dst[:rc].tobytes()


class CompressedInputStream:
    """K/io/CompressedInputStream.java: read() the whole decoded stream, or with from_block / to_block (the reference's context
    entries "from" / "to", :1193-1200: block ids from 1, `to` excluded) the blocks from_block .. to_block - 1, through
    kz_decompress_range."""

    def __init__(self, ctx, data, from_block=None, to_block=None):
        self.ctx, self.data = ctx, bytes(data)
        if (from_block is not None and from_block < 1) or (to_block is not None and to_block < (from_block or 1)):
            raise ValueError("from_block >= 1 and to_block >= from_block are needed")
        self.from_block, self.to_block = from_block, to_block

    def read(self, max_size=None):
        src = np.frombuffer(self.data + b"\0" * 16, dtype=np.uint8)
        cap = max_size if max_size is not None else self._declared_size()
        dst = np.empty(max(cap, 1), dtype=np.uint8)
        if self.from_block is None and self.to_block is None:
            rc = self.ctx.lib.kz_decompress(self.ctx.h, src.ctypes.data, len(self.data), dst.ctypes.data, cap)
        else:
            first = (self.from_block or 1) - 1
            count = _ALL_BLOCKS if self.to_block is None else self.to_block - 1 - first
            rc = self.ctx.lib.kz_decompress_range(self.ctx.h, src.ctypes.data, len(self.data), first, count, dst.ctypes.data, cap)
        self.ctx.check(rc)
        return dst[:rc].tobytes()

    def _declared_size(self):
        # The size field of the stream header is informative and untrusted (CompressedOutputStream.java:236-290): what the
        # stream can hold is bounded by its own block walk -- every block decodes to at most blockSize bytes.
        try:
            idx = knz_index(self.data)
            return max(len(idx["blocks"]) * idx["blockSize"], 1)
        except KanziError:
            pass
        # damaged stream: count the length prefixes that can still be walked (kz_decompress reports the fault itself)
        d, nbits = self.data, len(self.data) * 8
        if len(d) < 20:
            return 1 << 20
        v = int.from_bytes(d[:20], "big")
        block_size = ((v >> (160 - 119)) & ((1 << 28) - 1)) << 4
        szmask = (v >> (160 - 121)) & 3
        pos, nb = 121 + 16 * szmask + 15 + 24, 0

        def get(p, k):
            w = int.from_bytes(d[p // 8:(p + k + 7) // 8 + 1].ljust((k + 15) // 8 + 1, b"\0"), "big")
            tot = ((k + 15) // 8 + 1) * 8
            return (w >> (tot - (p % 8) - k)) & ((1 << k) - 1)
        while pos + 8 <= nbits and nb < (1 << 20):
            lr = get(pos, 5) + 3
            rd = get(pos + 5, lr)
            if rd == 0:
                break
            nb += 1
            pos += 5 + lr + rd
        return max((nb + 1) * max(min(block_size, 1 << 30), 1024), 1 << 20)


def knz_assemble(transform, entropy, block_size, input_size, streams, bits, checksum=0):
    """Host-only: build a .knz from per-block private streams (list of bytes) in block-id order.
    checksum = 0 / 32 / 64: what the block streams were coded with (Context.set_checksum)."""
    L = load_library()
    tt = transform if isinstance(transform, int) else transform_type(transform)
    et = entropy if isinstance(entropy, int) else ENTROPY_IDS[entropy.upper()]
    nb = len(streams)
    stride = max([len(s) for s in streams] + [8]) + 8
    buf = np.zeros(nb * stride + 8, dtype=np.uint8)
    for i, s in enumerate(streams):
        buf[i * stride:i * stride + len(s)] = np.frombuffer(s, dtype=np.uint8)
    b = np.ascontiguousarray(bits, dtype=np.int64)
    cap = int(sum((int(x) + 7) // 8 + 8 for x in bits)) + 64
    dst = np.zeros(cap, dtype=np.uint8)
    rc = L.kz_knz_assemble(tt, et, int(block_size), int(input_size), int(checksum), buf.ctypes.data, stride, b.ctypes.data, nb, dst.ctypes.data, cap)
    if rc < 0:
        raise KanziError(-rc, "knz_assemble")
    return dst[:rc].tobytes()


class KnzWriter:
    """Host-only streaming form of knz_assemble (kz_knz_writer_*): add() the block streams in block-id order as they arrive, close()
    -> the .knz bytes.  capacity: an upper bound of the stream's size (kz_compress_bound of the input is one)."""

    def __init__(self, transform, entropy, block_size, input_size, capacity, checksum=0):
        self.L = load_library()
        tt = transform if isinstance(transform, int) else transform_type(transform)
        et = entropy if isinstance(entropy, int) else ENTROPY_IDS[entropy.upper()]
        self.dst = np.zeros(int(capacity) + 64, dtype=np.uint8)
        self.w = self.L.kz_knz_writer_open(tt, et, int(block_size), int(input_size), int(checksum), self.dst.ctypes.data, len(self.dst))
        if not self.w:
            raise KanziError(18, "knz writer")

    def add(self, stream, bits):
        a = np.frombuffer(bytes(stream) + b"\0\0", dtype=np.uint8)
        rc = self.L.kz_knz_writer_add(self.w, a.ctypes.data, int(bits))
        if rc < 0:
            raise KanziError(-rc, "knz writer")

    def close(self):
        n = self.L.kz_knz_writer_close(self.w)
        self.w = None
        if n < 0:
            raise KanziError(-n, "knz writer")
        return self.dst[:n].tobytes()


def knz_index(data):
    """Host-only: -> dict(transform, entropy, blockSize, inputSize, blocks=[(bitOffset, bits), ...])."""
    L = load_library()
    src = np.frombuffer(bytes(data) + b"\0" * 16, dtype=np.uint8)
    tt, et, bs, isz, chk = ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)
    cap = len(data) * 8 // 9 + 16                 # a block takes 9 bits of the stream at the least (5 + 3 bit prefix, W >= 1)
    off = np.zeros(cap, dtype=np.int64)
    bits = np.zeros(cap, dtype=np.int64)
    nb = L.kz_knz_index(src.ctypes.data, len(data), ctypes.addressof(tt), ctypes.addressof(et), ctypes.addressof(bs),
                        ctypes.addressof(isz), ctypes.addressof(chk), off.ctypes.data, bits.ctypes.data, cap)
    if nb < 0:
        raise KanziError(-nb, "knz_index")
    return {"transform": tt.value, "entropy": et.value, "blockSize": bs.value, "inputSize": isz.value, "checksum": chk.value,
            "blocks": [(int(off[i]), int(bits[i])) for i in range(nb)]}


# ---- whole .knz stream on device memory (kz_compress_device and its kin: source and destination in HBM) ----
def compress_device(ctx, transform, entropy, block_size, src, n, dst, cap, checksum=0, skip_blocks=False):
    """kz_compress_device: the .knz stream of the n bytes at device address `src`, written at device address `dst` (capacity `cap`;
    compress_bound(n, block_size) always suffices) -> its size.  `src` / `dst`: integer device pointers, any alignment."""
    tt = transform if isinstance(transform, int) else transform_type(transform)
    et = entropy if isinstance(entropy, int) else ENTROPY_IDS[entropy.upper()]
    ctx.set_checksum(checksum)
    ctx.set_skip_blocks(skip_blocks)
    try:
        rc = ctx.lib.kz_compress_device(ctx.h, tt, et, int(block_size), _ptr(src), int(n), _ptr(dst), int(cap))
    finally:
        ctx.set_checksum(0)
        ctx.set_skip_blocks(False)
    return int(ctx.check(rc))


def decompress_device(ctx, src, n, dst, cap):
    """kz_decompress_device: decode the n-byte .knz stream at device address `src` into device address `dst` -> decoded size."""
    return int(ctx.check(ctx.lib.kz_decompress_device(ctx.h, _ptr(src), int(n), _ptr(dst), int(cap))))


def compress_bound(n, block_size):
    return int(load_library().kz_compress_bound(int(n), int(block_size)))


def knz_assemble_device(ctx, transform, entropy, block_size, input_size, streams, stride, bits, dst, cap, checksum=0):
    """kz_knz_assemble_device: knz_assemble with the rows (device address `streams`, `stride` bytes apart) and the destination on the
    device; `bits` is a host sequence, entries <= 0 are skipped -> the stream's size."""
    tt = transform if isinstance(transform, int) else transform_type(transform)
    et = entropy if isinstance(entropy, int) else ENTROPY_IDS[entropy.upper()]
    b = np.ascontiguousarray(bits, dtype=np.int64)
    rc = ctx.lib.kz_knz_assemble_device(ctx.h, tt, et, int(block_size), int(input_size), int(checksum), _ptr(streams), int(stride),
                                        b.ctypes.data if len(b) else None, len(b), _ptr(dst), int(cap))
    return int(ctx.check(rc))


def knz_index_device(ctx, src, n):
    """kz_knz_index_device: knz_index of the n-byte stream at device address `src` -> the same dict."""
    tt, et, bs, isz, chk = ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0)
    cap = int(n) * 8 // 9 + 16                    # a block takes 9 bits of the stream at the least (5 + 3 bit prefix, W >= 1)
    off = np.zeros(cap, dtype=np.int64)
    bits = np.zeros(cap, dtype=np.int64)
    nb = ctx.lib.kz_knz_index_device(ctx.h, _ptr(src), int(n), ctypes.addressof(tt), ctypes.addressof(et), ctypes.addressof(bs),
                                     ctypes.addressof(isz), ctypes.addressof(chk), off.ctypes.data, bits.ctypes.data, cap)
    if nb < 0:
        raise KanziError(-nb, "knz_index_device")
    return {"transform": tt.value, "entropy": et.value, "blockSize": bs.value, "inputSize": isz.value, "checksum": chk.value,
            "blocks": [(int(off[i]), int(bits[i])) for i in range(nb)]}


# ---- scan: the blocks of a stream found without the walk (kz_knz_scan / kz_knz_scan_device) ----
SCAN_END, SCAN_BROKEN = -1, -2


def _scan(call, head_bytes, n, min_chain, what):
    """call(minChain, header out-pointers ..., four arrays, cap, head) -> count; a second call when cap was too small"""
    tt, et, bs, isz, chk, head = ctypes.c_uint64(0), ctypes.c_uint32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
    cap = max(16, int(n) // 512)
    while True:
        cols = np.zeros((4, cap), dtype=np.int64)
        k = call(int(min_chain), ctypes.addressof(tt), ctypes.addressof(et), ctypes.addressof(bs), ctypes.addressof(isz), ctypes.addressof(chk),
                 cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data, cols[3].ctypes.data, cap, ctypes.addressof(head))
        if k < 0:
            raise KanziError(-k, what)
        if k <= cap:
            break
        cap = int(k)
    pre, off, bits, nxt = (cols[j][:k].tolist() for j in range(4))
    if head.value >= 0:
        header_bits = pre[head.value]                      # the entry behind the stream header starts where the header ends
    elif head_bytes is not None:
        header_bits = 160 + 16 * ((int.from_bytes(bytes(head_bytes[:20]), "big") >> 39) & 3)       # the 2-bit length of the size field, in 16-bit units
    else:
        header_bits = 160 + 16 * _size_field_units(isz.value)
    return {"transform": tt.value, "entropy": et.value, "blockSize": bs.value, "inputSize": isz.value, "checksum": chk.value,
            "blocks": list(zip(off, bits)), "prefix": pre, "next": nxt, "head": int(head.value),
            "headerBits": header_bits, "streamBits": 8 * int(n)}


def _size_field_units(n):
    """the 16-bit units of the stream header's size field that this library's writer (and the reference's) uses for n input bytes"""
    if n <= 0 or n >= 1 << 48:
        return 0
    if n >= 1 << 32:
        return 3
    units = 0
    if n > 1 << 30:
        n, units = n >> 4, 1
    return units + ((n.bit_length() - 1) >> 4) + 1


def knz_scan(data, min_chain=4):
    """kz_knz_scan (host only, no GPU): the blocks that a reader would accept at ANY bit position of the .knz bytes `data`, found without
    the walk and so behind damage as well -> knz_index's dict with "blocks" = the kept entries in ascending position, plus "prefix"
    (the bit where each entry's length prefix starts), "next" (the index of the entry that follows it in the stream, SCAN_END, or
    SCAN_BROKEN) and "head" (the entry behind the stream header, SCAN_END, or SCAN_BROKEN); "headerBits" and "streamBits" say where
    the stream header ends and the stream itself.  An entry is kept if it lies on a run of at least min_chain blocks, or if its run
    ends at the stream's end marker."""
    L = load_library()
    data = bytes(data)
    src = np.frombuffer(data + b"\0" * 16, dtype=np.uint8)
    return _scan(lambda mc, *a: L.kz_knz_scan(src.ctypes.data, len(data), mc, *a), data, len(data), min_chain, "knz_scan")


def knz_scan_device(ctx, src, n, min_chain=4, head_bytes=None):
    """kz_knz_scan_device: knz_scan of the n-byte stream at device address `src` -> the same dict.  "headerBits" is the position of
    the entry at "head"; for a scan whose head is SCAN_END or SCAN_BROKEN it is read from head_bytes, the stream's first 20 bytes,
    when the caller has them on the host (knz_salvage passes them), and is otherwise the header length that the writer gives a
    stream of this "inputSize"."""
    def call(mc, *a):
        k = ctx.lib.kz_knz_scan_device(ctx.h, _ptr(src), int(n), mc, *a)
        return int(ctx.check(k)) if k < 0 else k
    return _scan(call, head_bytes, n, min_chain, "knz_scan_device")


def knz_recover_index(scan):
    """What a scan (knz_scan / knz_scan_device) holds of the stream, in stream order; pure Python -> (entries, gaps).  The scan's
    entries are gone through in ascending prefix position; whenever one starts at or behind the end of what has been taken, its chain
    is followed by "next" to its end.  The last entry of a chain that ends SCAN_BROKEN counts as taken up to its payload's first bit
    only: the block in front of a break may be the damaged one, and then claims bits that are not its own (after a lost byte, the
    first bits of the next block).  The price: kept entries whose prefix lies INSIDE that last block's payload are taken as well,
    with their chains (a stream nested in it; chance hits at a small min_chain), and knz_salvage decodes them beside the block that
    holds them; inside a block of an unbroken chain such entries are passed over.  entries = the indices into the scan's lists in that order (on an intact stream: the chain from
    "head", which is kz_knz_index's list); gaps = [(first bit, end bit)] of what lies between the stream header and the stream's end
    and belongs to no taken entry: their prefixes, payloads and the final end marker do."""
    pre, blocks, nxt = scan["prefix"], scan["blocks"], scan["next"]
    entries, gaps = [], []
    pos = covered = scan["headerBits"]                     # entries in front of pos are passed over; bits in front of covered are taken
    end = scan["streamBits"]
    if not pre and scan["head"] == SCAN_END:
        return entries, gaps
    for i in range(len(pre)):
        if pre[i] < pos:
            continue
        if pre[i] > covered:
            gaps.append((covered, pre[i]))
        j = i
        while j >= 0:
            entries.append(j)
            pos = covered = max(covered, blocks[j][0] + blocks[j][1])
            if nxt[j] == SCAN_END:
                pos = covered = end
            elif nxt[j] == SCAN_BROKEN:
                pos = blocks[j][0]
            j = nxt[j]
    if covered < end:
        gaps.append((covered, end))
    return entries, gaps


def knz_salvage(ctx, knz, min_chain=4):
    """Everything that can still be read of a damaged .knz stream (bytes, or a torch.uint8 device tensor): scan it, put its chains in
    stream order (knz_recover_index) and decode them by index -> [(prefix bit, payload bit, bits, status, bytes or None)], one per
    recovered block in stream order; status is the block's own (0, or a negative code with None for its bytes).  The stream header
    must be whole; what lies between the recovered blocks is knz_recover_index's gaps."""
    if isinstance(knz, (bytes, bytearray, memoryview)):
        data = bytes(knz)
        scan = knz_scan(data, min_chain)
        entries, _ = knz_recover_index(scan)
        offs, bits = [scan["blocks"][i][0] for i in entries], [scan["blocks"][i][1] for i in entries]
        out, res = decode_indexed(ctx, data, offs, bits, stride=scan["blockSize"]) if entries else (None, None)
        rows = [out[k, :res[k].length].tobytes() if res[k].status == 0 else None for k in range(len(entries))]
    else:
        import torch
        src = knz.reshape(-1)
        torch.cuda.current_stream(src.device).synchronize()          # the calls run on the context's own stream
        scan = knz_scan_device(ctx, src.data_ptr(), src.numel(), min_chain, head_bytes=src[:20].cpu().numpy().tobytes())
        entries, _ = knz_recover_index(scan)
        offs, bits = [scan["blocks"][i][0] for i in entries], [scan["blocks"][i][1] for i in entries]
        rows = []
        if entries:
            bs = scan["blockSize"]
            out = torch.empty((len(entries), bs), dtype=torch.uint8, device=src.device)
            res = decode_indexed_device(ctx, src.data_ptr(), src.numel(), offs, bits, out.data_ptr(), bs)
            host = out.cpu().numpy()
            rows = [host[k, :res[k].length].tobytes() if res[k].status == 0 else None for k in range(len(entries))]
    return [(scan["prefix"][i], offs[k], bits[k], int(res[k].status), rows[k]) for k, i in enumerate(entries)]


def _byte_view(t):
    import torch
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("a contiguous device tensor is needed")
    return t.reshape(-1).view(torch.uint8)


def compress_tensor(ctx, t, transform="BWT+RANK+ZRLT", entropy="ANS0", block_size=4 << 20, checksum=0):
    """The .knz stream of a contiguous device tensor's bytes, as a torch.uint8 device tensor of exactly the stream's size.  The result
    is a VIEW of a buffer of compress_bound(nbytes, block_size) bytes, which stays allocated as long as the view lives: clone() it to
    keep only the stream."""
    import torch
    src = _byte_view(t)
    n = src.numel()
    cap = compress_bound(n, block_size)
    dst = torch.empty(cap, dtype=torch.uint8, device=t.device)
    torch.cuda.current_stream(t.device).synchronize()            # the call runs on the context's own stream
    size = compress_device(ctx, transform, entropy, block_size, src.data_ptr() if n else dst.data_ptr(), n, dst.data_ptr(), cap, checksum=checksum)
    return dst[:size]


def decompress_tensor(ctx, knz, out=None):
    """Decode a .knz stream held in a torch.uint8 device tensor -> a torch.uint8 device tensor of the decoded bytes (a view of `out`
    when given).  Without `out` the result is sized from the stream's own block walk (blocks x blockSize), not from the header's
    size field, which is informative and untrusted (CompressedInputStream._declared_size)."""
    import torch
    src = _byte_view(knz)
    n = src.numel()
    torch.cuda.current_stream(knz.device).synchronize()
    if out is None:
        idx = knz_index_device(ctx, src.data_ptr(), n)
        out = torch.empty(max(len(idx["blocks"]) * idx["blockSize"], 1), dtype=torch.uint8, device=knz.device)
    dst = _byte_view(out)
    size = decompress_device(ctx, src.data_ptr(), n, dst.data_ptr(), dst.numel())
    return dst[:size]


# ---- many .knz streams on device memory (kz_compress_many_device / kz_decompress_many_device) ----
def compress_many_bound(lengths, block_size):
    """kz_compress_many_bound: the sum of compress_bound(n, block_size) over `lengths`."""
    n = np.ascontiguousarray(lengths, dtype=np.int64)
    return int(load_library().kz_compress_many_bound(n.ctypes.data if len(n) else None, len(n), int(block_size)))


def _many_arrays(src_off, src_len, dst_off, dst_cap):
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (src_off, src_len, dst_off, dst_cap)]
    if len({len(a) for a in arrs}) != 1:
        raise ValueError("src_off, src_len, dst_off and dst_cap must have one length")
    return arrs


def compress_many_device(ctx, transform, entropy, block_size, src, src_off, src_len, dst, dst_off, dst_cap, checksum=0, skip_blocks=False):
    """kz_compress_many_device: stream s = the src_len[s] bytes at device address src + src_off[s], written into the slot at
    dst + dst_off[s] (capacity dst_cap[s]) -> a list with each stream's size, or its negative code (as kz_compress_device returns it
    for that buffer alone).  A fault of the call itself raises."""
    tt = transform if isinstance(transform, int) else transform_type(transform)
    et = entropy if isinstance(entropy, int) else ENTROPY_IDS[entropy.upper()]
    so, sl, do, dc = _many_arrays(src_off, src_len, dst_off, dst_cap)
    out = np.zeros(len(so), dtype=np.int64)
    ctx.set_checksum(checksum)
    ctx.set_skip_blocks(skip_blocks)
    try:
        rc = ctx.lib.kz_compress_many_device(ctx.h, tt, et, int(block_size), _ptr(src), so.ctypes.data, sl.ctypes.data, len(so),
                                             _ptr(dst), do.ctypes.data, dc.ctypes.data, out.ctypes.data)
    finally:
        ctx.set_checksum(0)
        ctx.set_skip_blocks(False)
    ctx.check(rc)
    return [int(v) for v in out]


def decompress_many_device(ctx, src, src_off, src_len, dst, dst_off, dst_cap):
    """kz_decompress_many_device: decode the src_len[s]-byte .knz stream at device address src + src_off[s] into the slot at
    dst + dst_off[s] (capacity dst_cap[s]) -> a list with each stream's decoded size, or its negative code."""
    so, sl, do, dc = _many_arrays(src_off, src_len, dst_off, dst_cap)
    out = np.zeros(len(so), dtype=np.int64)
    ctx.check(ctx.lib.kz_decompress_many_device(ctx.h, _ptr(src), so.ctypes.data, sl.ctypes.data, len(so),
                                                _ptr(dst), do.ctypes.data, dc.ctypes.data, out.ctypes.data))
    return [int(v) for v in out]


def compress_tensors(ctx, tensors, transform="BWT+RANK+ZRLT", entropy="ANS0", block_size=4 << 20, checksum=0):
    """compress_tensor for a list of contiguous device tensors in ONE call -> a list of torch.uint8 device tensors, one .knz stream
    per input.  They are views of one buffer of compress_many_bound bytes, which stays allocated as long as a view lives.  The inputs
    may lie in separate allocations.  A KanziError names the first tensor that failed."""
    import torch
    srcs = [_byte_view(t) for t in tensors]
    if not srcs:
        return []
    dev = srcs[0].device
    lens = [s.numel() for s in srcs]
    caps = [compress_bound(n, block_size) for n in lens]
    dst = torch.empty(compress_many_bound(lens, block_size), dtype=torch.uint8, device=dev)
    dst_off = [0] * len(caps)
    for i in range(1, len(caps)):
        dst_off[i] = dst_off[i - 1] + caps[i - 1]
    ptrs = [s.data_ptr() if n else dst.data_ptr() for s, n in zip(srcs, lens)]
    base = min(ptrs)                                             # offsets are relative to the lowest address
    torch.cuda.current_stream(dev).synchronize()                 # the call runs on the context's own stream
    sizes = compress_many_device(ctx, transform, entropy, block_size, base, [p - base for p in ptrs], lens,
                                 dst.data_ptr(), dst_off, caps, checksum=checksum)
    for i, sz in enumerate(sizes):
        if sz < 0:
            raise KanziError(-sz, "compress_tensors: tensor %d" % i)
    return [dst[o:o + sz] for o, sz in zip(dst_off, sizes)]


def decompress_tensors(ctx, streams, sizes=None):
    """Decode a list of .knz streams held in torch.uint8 device tensors in ONE call -> a list of torch.uint8 device tensors (views of
    one buffer).  sizes[i]: the capacity for stream i; without `sizes` each result is sized as decompress_tensor sizes it, from the
    stream's own block walk (blocks x blockSize) and not from the header's untrusted size field."""
    import torch
    srcs = [_byte_view(t) for t in streams]
    if not srcs:
        return []
    dev = srcs[0].device
    torch.cuda.current_stream(dev).synchronize()
    if sizes is None:
        sizes = []
        for s in srcs:
            idx = knz_index_device(ctx, s.data_ptr(), s.numel())
            sizes.append(len(idx["blocks"]) * idx["blockSize"])
    caps = [int(c) for c in sizes]
    dst_off = [0] * len(caps)
    for i in range(1, len(caps)):
        dst_off[i] = dst_off[i - 1] + caps[i - 1]
    dst = torch.empty(max(sum(caps), 1), dtype=torch.uint8, device=dev)
    ptrs = [s.data_ptr() if s.numel() else dst.data_ptr() for s in srcs]
    base = min(ptrs)
    got = decompress_many_device(ctx, base, [p - base for p in ptrs], [s.numel() for s in srcs], dst.data_ptr(), dst_off, caps)
    for i, sz in enumerate(got):
        if sz < 0:
            raise KanziError(-sz, "decompress_tensors: stream %d" % i)
    return [dst[o:o + sz] for o, sz in zip(dst_off, got)]


# ---- seekable streams: a block range (the reference's from / to), or blocks by an index ----
_ALL_BLOCKS = 1 << 62


def decompress_range(ctx, data, first, count, cap=None):
    """kz_decompress_range: blocks first .. first + count - 1 (numbered from 0) of the .knz bytes `data` -> their decoded bytes.  The
    prefixes in front of `first` are walked, so the cost grows with `first`; cap defaults to count blocks of the stream's size."""
    data = bytes(data)
    if cap is None:
        idx = knz_index(data)
        cap = max(min(int(count), max(len(idx["blocks"]) - int(first), 0)), 0) * idx["blockSize"]
    src = np.frombuffer(data + b"\0" * 16, dtype=np.uint8)
    dst = np.empty(max(int(cap), 1), dtype=np.uint8)
    rc = ctx.check(ctx.lib.kz_decompress_range(ctx.h, src.ctypes.data, len(data), int(first), int(count), dst.ctypes.data, int(cap)))
    return dst[:rc].tobytes()


def decompress_range_device(ctx, src, n, first, count, dst, cap):
    """kz_decompress_range_device: the same with the stream at device address `src` (n bytes) and the destination at device address
    `dst` (capacity cap) -> bytes produced."""
    return int(ctx.check(ctx.lib.kz_decompress_range_device(ctx.h, _ptr(src), int(n), int(first), int(count), _ptr(dst), int(cap))))


def _indexed(fn, ctx, src, n, offsets, bits, dst, stride):
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    w = np.ascontiguousarray(bits, dtype=np.int64)
    if len(off) != len(w):
        raise ValueError("offsets and bits differ in length")
    res = (BlockResult * max(len(off), 1))()
    ctx.check(fn(ctx.h, src, int(n), off.ctypes.data if len(off) else None, w.ctypes.data if len(w) else None, len(off),
                 dst, int(stride), ctypes.addressof(res)))
    return res


def decode_indexed(ctx, data, offsets, bits, stride=None):
    """kz_decode_indexed: the blocks of the .knz bytes `data` named by (bit offset, bit length) pairs as knz_index returns them, any
    subset in any order -> (uint8 array [len(offsets), stride], BlockResult array).  A block's fault is in its result's status; an
    entry that does not match the stream raises KanziError(18)."""
    data = bytes(data)
    if stride is None:
        stride = knz_index(data)["blockSize"]
    src = np.frombuffer(data + b"\0" * 16, dtype=np.uint8)
    out = np.zeros((len(offsets), int(stride)), dtype=np.uint8)
    res = _indexed(ctx.lib.kz_decode_indexed, ctx, src.ctypes.data, len(data), offsets, bits, out.ctypes.data if out.size else src.ctypes.data, stride)
    return out, res


def decode_indexed_device(ctx, src, n, offsets, bits, dst, stride):
    """kz_decode_indexed_device: the same with the stream at device address `src` (n bytes); block i goes to device address
    dst + i * stride -> BlockResult array (host)."""
    return _indexed(ctx.lib.kz_decode_indexed_device, ctx, _ptr(src), n, offsets, bits, _ptr(dst), stride)


# ---- byte-addressed reads: many ranges of the original data in one call (kz_read_bytes / kz_read_bytes_device) ----
def block_byte_offsets(input_sizes, block_size):
    """The blockByteOff table of a splice_concat of streams that kz_compress* wrote for inputs of the given sizes: every stream's
    blocks are block_size bytes but its last -> [0, ..., sum(input_sizes)], one entry more than the joined stream has blocks."""
    bs, out = int(block_size), [0]
    for n in input_sizes:
        n = int(n)
        if n < 0 or bs < 1:
            raise ValueError("sizes must not be negative")
        out += [out[-1] + min((k + 1) * bs, n) for k in range((n + bs - 1) // bs)]
    return out


def _read_arrays(index, offsets, sizes, byte_offsets):
    blocks = index["blocks"] if isinstance(index, dict) else list(index)
    off = np.ascontiguousarray([b[0] for b in blocks], dtype=np.int64)
    w = np.ascontiguousarray([b[1] for b in blocks], dtype=np.int64)
    ro = np.ascontiguousarray(offsets, dtype=np.int64)
    rl = np.ascontiguousarray(sizes, dtype=np.int64)
    if len(ro) != len(rl):
        raise ValueError("offsets and sizes differ in length")
    tab = None
    if byte_offsets is not None:
        tab = np.ascontiguousarray(byte_offsets, dtype=np.int64)
        if len(tab) != len(off) + 1:
            raise ValueError("byte_offsets needs one entry more than the index has blocks")
    return off, w, tab, ro, rl, np.zeros(max(len(ro), 1), dtype=np.int64)


def read_bytes(ctx, data, index, offsets, sizes, byte_offsets=None):
    """kz_read_bytes: bytes [offsets[i], offsets[i] + sizes[i]) of the original data of the .knz bytes `data`, for all i in one call
    -> (list of bytes, got).  index: knz_index(data) or its "blocks"; byte_offsets: where every block starts in the original data
    (block_byte_offsets), None for a stream whose blocks are all blockSize but the last.  A range is cut at the end of data;
    got[i] is its length, or the negative status of a block it touches (its entry in the list is then None)."""
    data = bytes(data)
    off, w, tab, ro, rl, got = _read_arrays(index, offsets, sizes, byte_offsets)
    src = np.frombuffer(data + b"\0" * 16, dtype=np.uint8)
    cap = int(rl.sum()) if len(rl) and int(rl.min()) >= 0 else 0
    dst = np.zeros(max(cap, 1), dtype=np.uint8)
    ctx.check(ctx.lib.kz_read_bytes(ctx.h, src.ctypes.data, len(data), _arg(off), _arg(w), None if tab is None else tab.ctypes.data, len(off),
                                    _arg(ro), _arg(rl), len(ro), dst.ctypes.data, cap, got.ctypes.data))
    at = np.concatenate(([0], np.cumsum(rl)))
    got = [int(g) for g in got[:len(ro)]]
    return [dst[at[i]:at[i] + g].tobytes() if g >= 0 else None for i, g in enumerate(got)], got


def read_bytes_device(ctx, src, n, index, offsets, sizes, dst, cap, byte_offsets=None):
    """kz_read_bytes_device: the same with the stream at device address `src` (n bytes); range i goes to device address
    dst + sum(sizes[:i]) (capacity `cap` >= sum(sizes)) -> got."""
    off, w, tab, ro, rl, got = _read_arrays(index, offsets, sizes, byte_offsets)
    ctx.check(ctx.lib.kz_read_bytes_device(ctx.h, _ptr(src), int(n), _arg(off), _arg(w), None if tab is None else tab.ctypes.data, len(off),
                                           _arg(ro), _arg(rl), len(ro), _ptr(dst), int(cap), got.ctypes.data))
    return [int(g) for g in got[:len(ro)]]


# ---- byte-addressed writes: many ranges of the original data replaced in one call (kz_write_bytes / kz_write_bytes_device) ----
def write_bytes_bound(index_bits, block_size):
    """kz_write_bytes_bound: a capacity that suffices for any write to a stream whose blocks have `index_bits` bits each."""
    b = np.ascontiguousarray(index_bits, dtype=np.int64)
    rc = int(load_library().kz_write_bytes_bound(b.ctypes.data if len(b) else None, len(b), int(block_size)))
    if rc < 0:
        raise KanziError(-rc, "write_bytes_bound")
    return rc


def _write_arrays(index, offsets, sizes, byte_offsets):
    off, w, tab, ro, rl, _ = _read_arrays(index, offsets, sizes, byte_offsets)
    new_off, new_w = np.zeros(max(len(off), 1), dtype=np.int64), np.zeros(max(len(off), 1), dtype=np.int64)
    return off, w, tab, ro, rl, new_off, new_w


def write_bytes(ctx, data, index, offsets, payloads, byte_offsets=None):
    """kz_write_bytes: the .knz bytes `data` with bytes [offsets[i], offsets[i] + len(payloads[i])) of its original data replaced by
    payloads[i], for all i in one call; where ranges overlap the later one wins -> (new stream, new index as knz_index names its
    blocks).  index: knz_index(data) or its "blocks"; byte_offsets: as for read_bytes.  Untouched blocks are copied bit for bit,
    touched ones are decoded, patched and encoded once; the data keeps its length."""
    data = bytes(data)
    payloads = [bytes(p) for p in payloads]
    off, w, tab, ro, rl, new_off, new_w = _write_arrays(index, offsets, [len(p) for p in payloads], byte_offsets)
    src = np.frombuffer(data + b"\0" * 16, dtype=np.uint8)
    new = np.frombuffer(b"".join(payloads) + b"\0", dtype=np.uint8)
    cap = write_bytes_bound(np.clip(w, 0, (1 << 34) - 1), knz_index(data)["blockSize"])
    dst = np.zeros(max(cap, 1), dtype=np.uint8)
    rc = ctx.check(ctx.lib.kz_write_bytes(ctx.h, src.ctypes.data, len(data), _arg(off), _arg(w), None if tab is None else tab.ctypes.data, len(off),
                                          _arg(ro), _arg(rl), len(ro), new.ctypes.data, len(new) - 1, dst.ctypes.data, cap, new_off.ctypes.data, new_w.ctypes.data))
    return dst[:rc].tobytes(), [(int(o), int(b)) for o, b in zip(new_off[:len(off)], new_w[:len(off)])]


def write_bytes_device(ctx, src, n, index, offsets, sizes, data, dst, cap, byte_offsets=None):
    """kz_write_bytes_device: the same with the stream at device address `src` (n bytes), range i's new bytes at device address
    data + sum(sizes[:i]) and the new stream written at device address `dst` (capacity `cap`; write_bytes_bound suffices)
    -> (the new stream's size, new index)."""
    off, w, tab, ro, rl, new_off, new_w = _write_arrays(index, offsets, sizes, byte_offsets)
    rc = ctx.check(ctx.lib.kz_write_bytes_device(ctx.h, _ptr(src), int(n), _arg(off), _arg(w), None if tab is None else tab.ctypes.data, len(off),
                                                 _arg(ro), _arg(rl), len(ro), _ptr(data), int(rl.sum()) if len(rl) else 0, _ptr(dst), int(cap),
                                                 new_off.ctypes.data, new_w.ctypes.data))
    return int(rc), [(int(o), int(b)) for o, b in zip(new_off[:len(off)], new_w[:len(off)])]


class KnzReader:
    """Random access to a .knz stream held as bytes or as a torch.uint8 device tensor: the index is built once (knz_index /
    knz_index_device, the one serial walk), every read after that goes through the indexed call and costs the same wherever its
    blocks lie.  Reads of a device stream return device tensors, reads of bytes return bytes.  byte_offsets (block_byte_offsets)
    says where every block starts in the original data, for read_many on a stream with short blocks in the middle."""

    def __init__(self, ctx, knz, byte_offsets=None):
        self.ctx = ctx
        self.byte_offsets = None if byte_offsets is None else [int(b) for b in byte_offsets]
        self.device = not isinstance(knz, (bytes, bytearray, memoryview))
        if self.device:
            import torch
            self.src = _byte_view(knz)
            torch.cuda.current_stream(knz.device).synchronize()      # the calls run on the context's own stream
            idx = knz_index_device(ctx, self.src.data_ptr(), self.src.numel())
        else:
            self.src = bytes(knz)
            idx = knz_index(self.src)
        self.index = idx
        self.block_size = idx["blockSize"]
        self.blocks = idx["blocks"]

    def _decode(self, ids):
        """-> (rows, results): rows[i] indexable by byte range, block_size apart"""
        ids = [int(i) for i in ids]
        for i in ids:
            if not 0 <= i < len(self.blocks):
                raise IndexError("block %d of %d" % (i, len(self.blocks)))
        offs, bits = [self.blocks[i][0] for i in ids], [self.blocks[i][1] for i in ids]
        if self.device:
            import torch
            out = torch.empty((max(len(ids), 1), self.block_size), dtype=torch.uint8, device=self.src.device)
            res = decode_indexed_device(self.ctx, self.src.data_ptr(), self.src.numel(), offs, bits, out.data_ptr(), self.block_size)
        else:
            out, res = decode_indexed(self.ctx, self.src, offs, bits, self.block_size)
        for k, i in enumerate(ids):
            if res[k].status:
                raise KanziError(-res[k].status, "block %d" % i)
        return out, res

    def read_blocks(self, ids):
        """the decoded blocks `ids` (any order, repeats allowed) -> a list of bytes, or of device tensors"""
        ids = list(ids)
        if not ids:
            return []
        out, res = self._decode(ids)
        return [out[k, :res[k].length] if self.device else out[k, :res[k].length].tobytes() for k in range(len(ids))]

    def read_at(self, offset, size):
        """bytes [offset, offset + size) of the original data (cut at its end, as a slice is).  Byte addresses are offset //
        blockSize: a covering block other than the stream's last that decodes to fewer than blockSize bytes raises KanziError."""
        offset, size = int(offset), int(size)
        if offset < 0 or size < 0:
            raise ValueError("offset and size must not be negative")
        bs, nb = self.block_size, len(self.blocks)
        b0, b1 = offset // bs, min((offset + size - 1) // bs, nb - 1)
        if size == 0 or b0 > b1:
            if self.device:
                import torch
                return torch.empty(0, dtype=torch.uint8, device=self.src.device)
            return b""
        out, res = self._decode(range(b0, b1 + 1))
        for k in range(b1 - b0 + 1):
            if res[k].length < bs and b0 + k != nb - 1:
                raise KanziError(15, "block %d decodes to %d bytes, fewer than the block size %d: the stream has no byte addressing"
                                 % (b0 + k, res[k].length, bs))
        have = (b1 - b0) * bs + res[b1 - b0].length               # bytes of the covering blocks, back to back in `out`
        lo, hi = offset - b0 * bs, min(offset - b0 * bs + size, have)
        flat = out.reshape(-1)
        if self.device:
            return flat[lo:max(hi, lo)].clone()
        return flat[lo:max(hi, lo)].tobytes()

    def read_many(self, offsets, sizes):
        """bytes [offsets[i], offsets[i] + sizes[i]) of the original data for all i, in one byte-addressed call (read_bytes /
        read_bytes_device): every covering block is decoded once -> a list of bytes, or of views into one packed device tensor.
        Each is cut at the end of data, as a slice is.  A range that touches a block that fails raises KanziError with that
        block's code."""
        offsets, sizes = [int(o) for o in offsets], [int(s) for s in sizes]
        if any(o < 0 for o in offsets) or any(s < 0 for s in sizes):
            raise ValueError("offset and size must not be negative")
        if self.device:
            import torch
            total = sum(sizes)
            out = torch.empty(max(total, 1), dtype=torch.uint8, device=self.src.device)
            got = read_bytes_device(self.ctx, self.src.data_ptr(), self.src.numel(), self.blocks, offsets, sizes, out.data_ptr(), total, self.byte_offsets)
        else:
            parts, got = read_bytes(self.ctx, self.src, self.blocks, offsets, sizes, self.byte_offsets)
        for i, g in enumerate(got):
            if g < 0:
                raise KanziError(-g, "range %d" % i)
        if not self.device:
            return parts
        res, at = [], 0
        for s, g in zip(sizes, got):
            res.append(out[at:at + g])
            at += s
        return res

    def write_many(self, offsets, payloads):
        """the stream with bytes [offsets[i], offsets[i] + len(payloads[i])) of its original data replaced by payloads[i] (bytes, or
        torch.uint8 tensors for a device stream), in one byte-addressed call (write_bytes / write_bytes_device); where ranges
        overlap the later one wins -> a new KnzReader on the new stream, with the same byte_offsets.  This reader is unchanged."""
        offsets = [int(o) for o in offsets]
        if len(offsets) != len(payloads):
            raise ValueError("offsets and payloads differ in length")
        if any(o < 0 for o in offsets):
            raise ValueError("offset must not be negative")
        if not self.device:
            new, _ = write_bytes(self.ctx, self.src, self.blocks, offsets, payloads, self.byte_offsets)
            return KnzReader(self.ctx, new, self.byte_offsets)
        import torch
        dev = self.src.device
        parts = [_byte_view(p).to(dev) if isinstance(p, torch.Tensor) else torch.from_numpy(np.frombuffer(bytes(p), dtype=np.uint8).copy()).to(dev) for p in payloads]
        sizes = [int(p.numel()) for p in parts]
        data = torch.cat(parts) if sum(sizes) else torch.zeros(1, dtype=torch.uint8, device=dev)
        cap = write_bytes_bound([b[1] for b in self.blocks], self.block_size)
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()                 # the call runs on the context's own stream
        size, _ = write_bytes_device(self.ctx, self.src.data_ptr(), self.src.numel(), self.blocks, offsets, sizes, data.data_ptr(), out.data_ptr(), cap, self.byte_offsets)
        return KnzReader(self.ctx, out[:size], self.byte_offsets)


# ---- many-stream index and byte-addressed reads (kz_knz_index_many_device / kz_read_bytes_many_device) ----
def knz_index_many_device(ctx, src, src_off, src_len):
    """kz_knz_index_many_device: knz_index_device for stream s = the src_len[s] bytes at device address src + src_off[s], all in one
    call -> a list with, per stream, the dict knz_index_device returns and "status" (its block count), or {"status": negative code}
    for a stream that fails.  A fault of the call itself raises."""
    so = np.ascontiguousarray(src_off, dtype=np.int64)
    sl = np.ascontiguousarray(src_len, dtype=np.int64)
    if len(so) != len(sl):
        raise ValueError("src_off and src_len must have one length")
    n = len(so)
    if n == 0:
        return []
    tt, et, bs = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    isz, chk, status, first = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int64)
    cap = max(16, int(sl.sum()) // 256)
    while True:
        off, bits = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64)
        total = int(ctx.check(ctx.lib.kz_knz_index_many_device(ctx.h, _ptr(src), so.ctypes.data, sl.ctypes.data, n, tt.ctypes.data, et.ctypes.data, bs.ctypes.data,
                                                               isz.ctypes.data, chk.ctypes.data, status.ctypes.data, first.ctypes.data, off.ctypes.data, bits.ctypes.data, cap)))
        if total <= cap:
            break
        cap = total                                             # a second call with that many
    out = []
    for s in range(n):
        if status[s] < 0:
            out.append({"status": int(status[s])})
            continue
        a, b = int(first[s]), int(first[s + 1])
        out.append({"status": int(status[s]), "transform": int(tt[s]), "entropy": int(et[s]), "blockSize": int(bs[s]), "inputSize": int(isz[s]), "checksum": int(chk[s]),
                    "blocks": [(int(o), int(w)) for o, w in zip(off[a:b], bits[a:b])]})
    return out


def _store_arrays(indices, byte_offsets):
    """indices: per stream its blocks [(bit offset, bits)] (or the dict that holds them, or None for a stream without an index);
    byte_offsets: None, or per stream None / its table -> (indexFirst, blockBitOff, blockBits, tableFirst or None, blockByteOff or None)"""
    blocks = [[] if i is None else (i.get("blocks", []) if isinstance(i, dict) else list(i)) for i in indices]
    first = np.zeros(len(blocks) + 1, dtype=np.int64)
    first[1:] = np.cumsum([len(b) for b in blocks])
    off = np.ascontiguousarray([b[0] for bl in blocks for b in bl], dtype=np.int64)
    w = np.ascontiguousarray([b[1] for bl in blocks for b in bl], dtype=np.int64)
    if byte_offsets is None or all(t is None for t in byte_offsets):
        return first, off, w, None, None
    if len(byte_offsets) != len(blocks):
        raise ValueError("byte_offsets needs one entry per stream")
    tfirst, tab = np.full(len(blocks), -1, dtype=np.int64), []
    for s, t in enumerate(byte_offsets):
        if t is None:
            continue
        if len(t) != len(blocks[s]) + 1:
            raise ValueError("byte_offsets[%d] needs one entry more than the stream has blocks" % s)
        tfirst[s] = len(tab)
        tab += [int(x) for x in t]
    return first, off, w, tfirst, np.ascontiguousarray(tab, dtype=np.int64)


def read_bytes_many_device(ctx, src, src_off, src_len, indices, streams, offsets, sizes, dst, cap, byte_offsets=None):
    """kz_read_bytes_many_device: range i = bytes [offsets[i], offsets[i] + sizes[i]) of the original data of stream streams[i]
    (stream s = the src_len[s] bytes at device address src + src_off[s]); it goes to device address dst + sum(sizes[:i]) (capacity
    `cap` >= sum(sizes)).  indices: per stream its index as knz_index_many_device returns it (or its "blocks"); byte_offsets: None, or
    per stream None / its table of block starts -> (got, stream status), lists of ints."""
    so = np.ascontiguousarray(src_off, dtype=np.int64)
    sl = np.ascontiguousarray(src_len, dtype=np.int64)
    if not len(so) == len(sl) == len(indices):
        raise ValueError("src_off, src_len and indices must have one length")
    first, off, w, tfirst, tab = _store_arrays(indices, byte_offsets)
    rs = np.ascontiguousarray(streams, dtype=np.int32)
    ro = np.ascontiguousarray(offsets, dtype=np.int64)
    rl = np.ascontiguousarray(sizes, dtype=np.int64)
    if not len(rs) == len(ro) == len(rl):
        raise ValueError("streams, offsets and sizes differ in length")
    got, status = np.zeros(max(len(ro), 1), dtype=np.int64), np.zeros(max(len(so), 1), dtype=np.int32)
    ctx.check(ctx.lib.kz_read_bytes_many_device(ctx.h, _ptr(src), _arg(so), _arg(sl), len(so), first.ctypes.data, _arg(off), _arg(w),
                                                None if tfirst is None else tfirst.ctypes.data, None if tab is None else _arg(tab),
                                                _arg(rs), _arg(ro), _arg(rl), len(ro), _ptr(dst), int(cap), got.ctypes.data, status.ctypes.data))
    return [int(g) for g in got[:len(ro)]], [int(c) for c in status[:len(so)]]


# ---- many-stream byte-addressed writes (kz_write_bytes_many_bound / kz_write_bytes_many_device) ----
def write_bytes_many_bound(indices, block_sizes):
    """kz_write_bytes_many_bound: per stream a slot capacity that suffices for any write to it (write_bytes_bound of its index and
    block size) -> (their sum, the list of capacities)."""
    first, _, w, _, _ = _store_arrays(indices, None)
    bs = np.ascontiguousarray(block_sizes, dtype=np.int32)
    if len(bs) != len(first) - 1:
        raise ValueError("indices and block_sizes must have one length")
    caps = np.zeros(max(len(bs), 1), dtype=np.int64)
    bits = np.ascontiguousarray(np.clip(w, 0, (1 << 34) - 1), dtype=np.int64)
    rc = int(load_library().kz_write_bytes_many_bound(first.ctypes.data, _arg(bits), _arg(bs), len(bs), caps.ctypes.data))
    if rc < 0:
        raise KanziError(-rc, "write_bytes_many_bound")
    return rc, [int(x) for x in caps[:len(bs)]]


def write_bytes_many_device(ctx, src, src_off, src_len, indices, streams, offsets, sizes, data, dst, dst_off, dst_cap, byte_offsets=None):
    """kz_write_bytes_many_device: range i = bytes [offsets[i], offsets[i] + sizes[i]) of the original data of stream streams[i]
    (stream s = the src_len[s] bytes at device address src + src_off[s]) is replaced by the sizes[i] bytes at device address data +
    sum(sizes[:i]); the new stream s goes to device address dst + dst_off[s] (capacity dst_cap[s]; write_bytes_many_bound suffices).
    indices, byte_offsets: as for read_bytes_many_device -> (dst_len, new_indices): per stream the new stream's size, 0 for a stream
    that no range names or its negative code, and its new index (None unless the stream was written)."""
    so = np.ascontiguousarray(src_off, dtype=np.int64)
    sl = np.ascontiguousarray(src_len, dtype=np.int64)
    do = np.ascontiguousarray(dst_off, dtype=np.int64)
    dc = np.ascontiguousarray(dst_cap, dtype=np.int64)
    if not len(so) == len(sl) == len(indices) == len(do) == len(dc):
        raise ValueError("src_off, src_len, indices, dst_off and dst_cap must have one length")
    first, off, w, tfirst, tab = _store_arrays(indices, byte_offsets)
    rs = np.ascontiguousarray(streams, dtype=np.int32)
    ro = np.ascontiguousarray(offsets, dtype=np.int64)
    rl = np.ascontiguousarray(sizes, dtype=np.int64)
    if not len(rs) == len(ro) == len(rl):
        raise ValueError("streams, offsets and sizes differ in length")
    n = len(so)
    dl = np.zeros(max(n, 1), dtype=np.int64)
    new_off, new_w = np.zeros(max(len(off), 1), dtype=np.int64), np.zeros(max(len(off), 1), dtype=np.int64)
    ctx.check(ctx.lib.kz_write_bytes_many_device(ctx.h, _ptr(src), _arg(so), _arg(sl), n, first.ctypes.data, _arg(off), _arg(w),
                                                 None if tfirst is None else tfirst.ctypes.data, None if tab is None else _arg(tab),
                                                 _arg(rs), _arg(ro), _arg(rl), len(ro), _ptr(data), int(rl.sum()) if len(rl) else 0,
                                                 _ptr(dst), _arg(do), _arg(dc), dl.ctypes.data, new_off.ctypes.data, new_w.ctypes.data))
    dst_len = [int(x) for x in dl[:n]]
    new = [[(int(o), int(b)) for o, b in zip(new_off[int(first[s]):int(first[s + 1])], new_w[int(first[s]):int(first[s + 1])])] if dst_len[s] > 0 else None
           for s in range(n)]
    return dst_len, new


class KnzStore:
    """Many .knz streams in one torch.uint8 device tensor (what compress_many_device leaves behind), read by byte address: the
    indices of all streams come from ONE knz_index_many_device call, every read after that is one read_bytes_many_device call over
    records of any of the streams.  byte_offsets: None, or per stream None / its table of block starts (block_byte_offsets), for
    streams with short blocks in the middle.  A stream that cannot be indexed is kept with its code (status[s] < 0) and fails the
    reads that name it."""

    def __init__(self, ctx, buf, src_off, src_len, byte_offsets=None):
        import torch
        self.ctx = ctx
        self.src = _byte_view(buf)
        self.src_off = [int(o) for o in src_off]
        self.src_len = [int(n) for n in src_len]
        if len(self.src_off) != len(self.src_len):
            raise ValueError("src_off and src_len must have one length")
        for o, n in zip(self.src_off, self.src_len):
            if o < 0 or n < 0 or o + n > self.src.numel():
                raise ValueError("a stream lies outside the buffer")
        self.byte_offsets = None if byte_offsets is None else [None if t is None else [int(b) for b in t] for t in byte_offsets]
        torch.cuda.current_stream(self.src.device).synchronize()     # the calls run on the context's own stream
        self.index = knz_index_many_device(ctx, self.src.data_ptr(), self.src_off, self.src_len)
        self.status = [i["status"] for i in self.index]

    @classmethod
    def from_compress_many(cls, ctx, dst, dst_off, sizes, byte_offsets=None):
        """the store of the streams that compress_many_device wrote into the tensor `dst`: its dst_off argument and its result"""
        for s, n in enumerate(sizes):
            if n < 0:
                raise KanziError(-n, "KnzStore: stream %d was not written" % s)
        return cls(ctx, dst, dst_off, sizes, byte_offsets)

    def __len__(self):
        return len(self.src_off)

    def read_many(self, streams, offsets, sizes, out=None):
        """bytes [offsets[i], offsets[i] + sizes[i]) of the original data of stream streams[i] for all i in one call -> (packed, got):
        record i is packed[sum(sizes[:i]) :][:got[i]], cut at the end of its stream's data as a slice is.  out: a torch.uint8 device
        tensor of at least sum(sizes) bytes to write into.  A record of a stream or a block that fails raises KanziError."""
        import torch
        streams, offsets, sizes = [int(s) for s in streams], [int(o) for o in offsets], [int(n) for n in sizes]
        if not len(streams) == len(offsets) == len(sizes):
            raise ValueError("streams, offsets and sizes differ in length")
        if any(o < 0 for o in offsets) or any(n < 0 for n in sizes):
            raise ValueError("offset and size must not be negative")
        if any(not 0 <= s < len(self) for s in streams):
            raise IndexError("stream out of range")
        total = sum(sizes)
        if out is None:
            out = torch.empty(max(total, 1), dtype=torch.uint8, device=self.src.device)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < total or out.device != self.src.device:
            raise ValueError("out must be a contiguous torch.uint8 tensor of sum(sizes) bytes on the store's device")
        torch.cuda.current_stream(self.src.device).synchronize()
        got, _ = read_bytes_many_device(self.ctx, self.src.data_ptr(), self.src_off, self.src_len, self.index, streams, offsets, sizes,
                                        out.data_ptr(), total, self.byte_offsets)
        for i, g in enumerate(got):
            if g < 0:
                raise KanziError(-g, "range %d (stream %d)" % (i, streams[i]))
        return out[:total], got

    def read(self, stream, off, size):
        """bytes [off, off + size) of the original data of one stream -> a device tensor"""
        out, got = self.read_many([stream], [off], [size])
        return out[:got[0]]

    def write_many(self, streams, offsets, payloads):
        """the store with bytes [offsets[i], offsets[i] + len(payloads[i])) of the original data of stream streams[i] replaced by
        payloads[i] (bytes, or torch.uint8 tensors) for all i in ONE write_bytes_many_device call; where ranges of a stream overlap
        the later one wins -> a NEW KnzStore in a tensor of its own, with the same byte_offsets: the streams that no record names are
        copied verbatim.  This store is unchanged.  A stream that fails raises KanziError."""
        import torch
        streams, offsets = [int(s) for s in streams], [int(o) for o in offsets]
        if not len(streams) == len(offsets) == len(payloads):
            raise ValueError("streams, offsets and payloads differ in length")
        if any(o < 0 for o in offsets):
            raise ValueError("offset must not be negative")
        if any(not 0 <= s < len(self) for s in streams):
            raise IndexError("stream out of range")
        dev = self.src.device
        is_named = set(streams)
        named = sorted(is_named)
        for s in named:
            if self.status[s] < 0:
                raise KanziError(-self.status[s], "KnzStore: stream %d has no index" % s)
        parts = [_byte_view(p).to(dev) if isinstance(p, torch.Tensor) else torch.from_numpy(np.frombuffer(bytes(p), dtype=np.uint8).copy()).to(dev) for p in payloads]
        sizes = [int(p.numel()) for p in parts]
        data = torch.cat(parts) if sum(sizes) else torch.zeros(1, dtype=torch.uint8, device=dev)
        indices = [self.index[s] if s in is_named else None for s in range(len(self))]
        _, caps = write_bytes_many_bound(indices, [self.index[s]["blockSize"] if s in is_named else 1024 for s in range(len(self))])
        dst_off, dst_cap, at = [], [], 0
        for s in range(len(self)):                                   # a slot of the bound for a named stream, of its own size for every other
            cap = caps[s] if s in is_named else self.src_len[s]
            dst_off.append(at)
            dst_cap.append(cap)
            at += cap
        out = torch.empty(max(at, 1), dtype=torch.uint8, device=dev)
        for s in range(len(self)):
            if s not in is_named and self.src_len[s]:
                out[dst_off[s]:dst_off[s] + self.src_len[s]] = self.src[self.src_off[s]:self.src_off[s] + self.src_len[s]]
        torch.cuda.current_stream(dev).synchronize()                 # the call runs on the context's own stream
        dst_len, _ = write_bytes_many_device(self.ctx, self.src.data_ptr(), self.src_off, self.src_len, indices, streams, offsets, sizes,
                                             data.data_ptr(), out.data_ptr(), dst_off, dst_cap,
                                             None if self.byte_offsets is None else [t if s in is_named else None for s, t in enumerate(self.byte_offsets)])
        for s in named:
            if dst_len[s] < 0:
                raise KanziError(-dst_len[s], "KnzStore.write_many: stream %d: %s" % (s, self.ctx.error()))
        new_len = [dst_len[s] if s in is_named else self.src_len[s] for s in range(len(self))]
        return KnzStore(self.ctx, out, dst_off, new_len, self.byte_offsets)

    def write(self, stream, off, payload):
        """the one-record form of write_many -> a new KnzStore"""
        return self.write_many([stream], [off], [payload])


# ---- splice: a new .knz stream out of blocks of existing ones, without recoding (kz_knz_splice / kz_knz_splice_device) ----
def knz_splice_bound(bits):
    """kz_knz_splice_bound: a capacity that suffices for a splice of pieces of `bits` bits each."""
    b = np.ascontiguousarray(bits, dtype=np.int64)
    rc = int(load_library().kz_knz_splice_bound(b.ctypes.data if len(b) else None, len(b)))
    if rc < 0:
        raise KanziError(-rc, "knz_splice_bound")
    return rc


def _piece_arrays(pieces):
    ps = np.ascontiguousarray([p[0] for p in pieces], dtype=np.int32)
    po = np.ascontiguousarray([p[1] for p in pieces], dtype=np.int64)
    pw = np.ascontiguousarray([p[2] for p in pieces], dtype=np.int64)
    return ps, po, pw


def _arg(a):
    return a.ctypes.data if len(a) else None


def knz_splice(sources, pieces, input_size, cap=None):
    """kz_knz_splice (host memory, no GPU): the stream made of `pieces` = [(source, bitOff, bits)], blocks of the .knz streams in
    `sources` (a list of bytes) named as knz_index names them, in this order; the header parameters are the sources' own, which must
    agree, and `input_size` goes into the header's size field (0: unknown) -> the stream's bytes.  Blocks are not decoded."""
    L = load_library()
    sources = [bytes(s) for s in sources]
    ps, po, pw = _piece_arrays(pieces)
    so = np.zeros(len(sources), dtype=np.int64)
    sl = np.ascontiguousarray([len(s) for s in sources], dtype=np.int64)
    if len(sources) > 1:
        so[1:] = np.cumsum(sl)[:-1]
    src = np.frombuffer(b"".join(sources) + b"\0", dtype=np.uint8)
    if cap is None:
        cap = knz_splice_bound(np.clip(pw, 0, (1 << 34) - 1))
    dst = np.zeros(max(int(cap), 1), dtype=np.uint8)
    rc = L.kz_knz_splice(src.ctypes.data, _arg(so), _arg(sl), len(sources), _arg(ps), _arg(po), _arg(pw), len(ps), int(input_size), dst.ctypes.data, int(cap))
    if rc < 0:
        raise KanziError(-rc, "knz_splice")
    return dst[:rc].tobytes()


def knz_splice_device(ctx, src, src_off, src_len, pieces, input_size, dst, cap):
    """kz_knz_splice_device: the same with source s the src_len[s] bytes at device address src + src_off[s] and the result written at
    device address `dst` (capacity `cap`; knz_splice_bound of the pieces' bits suffices) -> the stream's size.  The payload bits go
    from the sources to their place in `dst` in one kernel per chunk of pieces; nothing is staged or recoded."""
    ps, po, pw = _piece_arrays(pieces)
    so = np.ascontiguousarray(src_off, dtype=np.int64)
    sl = np.ascontiguousarray(src_len, dtype=np.int64)
    if len(so) != len(sl):
        raise ValueError("src_off and src_len differ in length")
    rc = ctx.lib.kz_knz_splice_device(ctx.h, _ptr(src), _arg(so), _arg(sl), len(so), _arg(ps), _arg(po), _arg(pw), len(ps), int(input_size), _ptr(dst), int(cap))
    return int(ctx.check(rc))


def _decoded_size(index):
    """(size, known) of an indexed stream under the planners' rule: every block decodes to blockSize bytes except the stream's
    last, whose length is what the header's size field leaves; known is False when the header carries no size or one that does not
    fit that rule"""
    nb, bs, n = len(index["blocks"]), index["blockSize"], index["inputSize"]
    if nb == 0:
        return 0, n == 0
    return n, (nb - 1) * bs < n <= nb * bs


def splice_concat(indices):
    """Plan of the join of whole streams: indices[s] = knz_index of source s -> (pieces, input_size) for knz_splice /
    knz_splice_device.  input_size is the sum of the sources' header sizes.  The result is the stream the compressor writes for the
    joined data only if every source but the last holds whole blocks; otherwise it still decodes to the joined data, with short
    blocks in the middle.  Sizes are taken as "every block blockSize except a stream's last", which holds for the streams
    kz_compress* wrote and not for ones with short middle blocks or without a size in their header: then input_size is 0 (unknown)."""
    pieces, total, known = [], 0, True
    for s, idx in enumerate(indices):
        pieces += [(s, off, w) for off, w in idx["blocks"]]
        n, k = _decoded_size(idx)
        total, known = total + n, known and k
    return pieces, (total if known else 0)


def splice_slice(index, first, count):
    """Plan of blocks [first, first + count) of one stream as a stream of its own -> (pieces, input_size); the same rule for sizes as
    splice_concat, 0 (unknown) where it does not hold."""
    nb, bs = len(index["blocks"]), index["blockSize"]
    first = max(int(first), 0)
    last = min(first + max(int(count), 0), nb)
    pieces = [(0, off, w) for off, w in index["blocks"][first:last]]
    n, known = _decoded_size(index)
    if not known:
        return pieces, 0
    return pieces, max(min(last * bs, n) - first * bs, 0)


def splice_replace(index, k, other_source, other_index):
    """Plan of source 0 (index) with its block k replaced by all blocks of source `other_source` (other_index: its knz_index, as a
    rule one freshly compressed block); k == number of blocks appends -> (pieces, input_size); the same rule for sizes as
    splice_concat, 0 (unknown) where it does not hold, for instance when a short block comes to lie in the middle."""
    blocks, bs = index["blocks"], index["blockSize"]
    k = int(k)
    if not 0 <= k <= len(blocks):
        raise IndexError("block %d of %d" % (k, len(blocks)))
    new = [(int(other_source), off, w) for off, w in other_index["blocks"]]
    pieces = [(0, off, w) for off, w in blocks[:k]] + new + [(0, off, w) for off, w in blocks[k + 1:]]
    n, known = _decoded_size(index)
    m, mknown = _decoded_size(other_index)
    lens = [min(bs, n - i * bs) for i in range(len(blocks))]
    olens = [min(bs, m - i * bs) for i in range(len(other_index["blocks"]))]
    out = lens[:k] + olens + lens[k + 1:]
    if not (known and mknown) or any(l != bs for l in out[:-1]):
        return pieces, 0
    return pieces, sum(out)


def usable_cpus():
    """CPUs this process can actually use: its affinity mask cut down to the cgroup CPU quota, if any (kz_host.hip)."""
    return int(load_library().kz_host_cpus())


def pin_host_threads_to_gpu(device, world=2):
    """One process per GPU, `world` of them on one host: keep this process's host threads (TEXT / UTF stages, bit assembly,
    staging copies) on the CPUs of the GPU's NUMA node, and its thread pool inside 1/world of the host's CPU quota.  A single process (world == 1) keeps the whole machine.  Returns the
    number of CPUs pinned to (0: nothing changed)."""
    if world <= 1:
        return 0
    lib = load_library()
    lib.kz_host_share(int(world))                 # and 1/world of the cgroup CPU quota, if there is one
    return max(0, int(lib.kz_pin_to_device_numa(int(device))))


def shard_blocks(n_blocks, world, rank):
    """Round-robin block partition over GPUs: block i -> rank i mod world."""
    return list(range(rank, n_blocks, world))


def extract_bits(data, bit_off, nbits):
    """Host helper: the nbits-long bit string starting at bit_off of `data`, left aligned (MSB first)."""
    v = int.from_bytes(data[bit_off // 8:(bit_off + nbits + 7) // 8 + 1], "big")
    total = ((bit_off + nbits + 7) // 8 + 1 - bit_off // 8) * 8
    have = min(total, len(data) * 8 - (bit_off // 8) * 8)
    v <<= (total - have)
    v = (v >> (total - (bit_off % 8) - nbits)) & ((1 << nbits) - 1)
    pad = (-nbits) % 8
    return (v << pad).to_bytes((nbits + 7) // 8, "big")
