"""zsamd -- Python host binding of the MI355X batched deflate/inflate engine.

Mirrors the reference's public surface (src/streams-api.ts, src/mod/streams.ts):

* ``CompressionStream(format, level=...)`` / ``DecompressionStream(format)`` with
  ``write()`` / ``close()`` / ``read()`` -- one stream, run as a batch of one.
* ``compress_batch(inputs, format, level)`` / ``decompress_batch(inputs, format)``
  -- the batch entry the north star adds to ``streams-api.ts``; stream i yields
  exactly what piping ``inputs[i]`` alone through the reference stream class
  (one ``write()`` then ``close()``) yields, or raises/reports the same error.

Everything runs on the GPU through the C-ABI in ``libzsgpu.so``
(include/zs_gpu.h).  There is no CPU fallback: if the library or a GPU is
missing, every entry point raises ``ZsUnavailable``.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZS_LIB overrides the library path (A/B runs of kernel variants)
LIB_PATH = os.environ.get("ZS_LIB") or os.path.join(os.path.dirname(_HERE), "libzsgpu.so")

Z_OK, Z_STREAM_END, Z_NEED_DICT = 0, 1, 2
Z_STREAM_ERROR, Z_DATA_ERROR, Z_MEM_ERROR, Z_BUF_ERROR = -2, -3, -4, -5
PHASE_NONE, PHASE_INIT, PHASE_PROCESS, PHASE_FINISH = 0, 1, 2, 3
# deflateInit2_'s strategy (deflate.ts:289-290, :923-931; ZS_* in zs_gpu.h)
Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 0, 1, 2, 3, 4

# format -> windowBits, streams.ts:220 (compression) and :233 (decompression).
# Unknown strings fall through to 15 there ("deflate"); the same here.
def compress_wbits(fmt: str) -> int:
    return 31 if fmt == "gzip" else (-15 if fmt == "deflate-raw" else 15)


def decompress_wbits(fmt: str) -> int:
    if fmt == "gzip":
        return 31
    if fmt == "deflate-raw":
        return -15
    if fmt == "deflate64-raw":
        return -16
    return 15


class ZsUnavailable(RuntimeError):
    """The HIP engine (libzsgpu.so) or a GPU is not available."""


class ZsError(Exception):
    """Mirrors the Error the reference stream layer throws (streams.ts:53,117,170)."""

    def __init__(self, message: str, status: int = 0, phase: int = 0, msg: str = ""):
        super().__init__(message)
        self.status, self.phase, self.msg = status, phase, msg


def compress_level(level) -> int:
    """streams.ts:221: a level that is not a number means Z_DEFAULT_COMPRESSION (-1, deflate.ts:268-270)."""
    if isinstance(level, bool) or not isinstance(level, int):
        return -1
    return level


def compress_strategy(strategy, zdict=None) -> int:
    """The `strategy` keyword of the compress entries: 0..4 (Z_DEFAULT_STRATEGY .. Z_FIXED);
    anything else is deflateInit2_'s Z_STREAM_ERROR (deflate.ts:289-290), reported as the
    stream layer does ("init failed: -2", streams.ts:53).  A strategy other than 0 together
    with a preset dictionary is not built (zs_gpu.h): ValueError, before any call."""
    if isinstance(strategy, bool) or not isinstance(strategy, int) or not 0 <= strategy <= Z_FIXED:
        raise ZsError("init failed: %d" % Z_STREAM_ERROR, Z_STREAM_ERROR, PHASE_INIT, "invalid strategy")
    if strategy and zdict is not None:
        raise ValueError("strategy %d with a preset dictionary is not built" % strategy)
    return strategy


def compress_params(fmt: str, window_bits=None, mem_level=8, zdict=None, strategy=0) -> int:
    """The `window_bits` (8..15; None = 15) and `mem_level` (1..9) keywords of the compress entries:
    deflateInit2_'s windowBits and memLevel (deflate.ts:253-343).  Returns the windowBits code of
    the zs_deflate_batch_params entries: -window_bits for "deflate-raw", window_bits + 16 for
    "gzip", window_bits for "deflate".  Values deflateInit2_ refuses (deflate.ts:281-294: not an
    int, out of range, 8 for deflate-raw or gzip) raise ZsError("init failed: -2"), as the stream
    layer reports them (streams.ts:53).  Parameters other than 15 / 8 together with a preset
    dictionary or a strategy are not built (zs_gpu.h): ValueError, before any call."""
    wb = 15 if window_bits is None else window_bits
    if isinstance(wb, bool) or not isinstance(wb, int) or not 8 <= wb <= 15 or (wb == 8 and fmt in ("deflate-raw", "gzip")):
        raise ZsError("init failed: %d" % Z_STREAM_ERROR, Z_STREAM_ERROR, PHASE_INIT, "invalid window bits")
    if isinstance(mem_level, bool) or not isinstance(mem_level, int) or not 1 <= mem_level <= 9:
        raise ZsError("init failed: %d" % Z_STREAM_ERROR, Z_STREAM_ERROR, PHASE_INIT, "invalid memLevel")
    if wb != 15 or mem_level != 8:
        if zdict is not None:
            raise ValueError("window_bits %d / mem_level %d with a preset dictionary is not built" % (wb, mem_level))
        if strategy:
            raise ValueError("window_bits %d / mem_level %d with strategy %d is not built" % (wb, mem_level, strategy))
    return -wb if fmt == "deflate-raw" else wb + 16 if fmt == "gzip" else wb


Z_FULL_FLUSH = 3  # deflate()'s flush argument (ZS_FULL_FLUSH in zs_gpu.h)


def compress_flush(lens, flush_at=None, flush_every=None, zdict=None, strategy=0, window_bits=None, mem_level=8):
    """The `flush_at` / `flush_every` keywords of the compress entries: Z_FULL_FLUSH points
    (zs_deflate_batch_flush; deflate.ts:942-961).  flush_at: one list of positions for every
    stream, or one list per stream (None / empty = none); flush_every=N: the positions N, 2N, ...
    below each stream's length.  Returns None without either, else a list of position lists, one
    per stream.  Together with zdict, a strategy or parameters other than 15 / 8 they are not
    built (zs_gpu.h): ValueError, before any call.  Positions the entry refuses (not increasing,
    past the length) are its ZS_STREAM_ERROR."""
    if flush_at is None and flush_every is None:
        return None
    if flush_at is not None and flush_every is not None:
        raise ValueError("flush_at and flush_every are alternatives")
    if zdict is not None:
        raise ValueError("flush points with a preset dictionary are not built")
    if strategy:
        raise ValueError("flush points with strategy %d are not built" % strategy)
    if not _params_default(window_bits, mem_level):
        raise ValueError("flush points with window_bits / mem_level are not built")
    n = len(lens)
    if flush_every is not None:
        if isinstance(flush_every, bool) or not isinstance(flush_every, int) or flush_every <= 0:
            raise ValueError("flush_every must be a positive int")
        return [list(range(flush_every, ln, flush_every)) for ln in lens]
    fa = list(flush_at)
    if all(isinstance(x, int) and not isinstance(x, bool) for x in fa):  # (an empty list: no points)
        per = [fa] * n
    else:
        per = [[] if x is None else list(x) for x in fa]
        if len(per) != n:
            raise ValueError("flush_at: %d position lists for %d inputs" % (len(per), n))
    for ps in per:
        for x in ps:
            if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x <= 0xffffffff:
                raise ValueError("flush_at: positions are ints in 0 .. 2^32 - 1")
    return per


def compress_primed(primed, flush_at=None, flush_every=None, bgzf=None) -> bool:
    """The `primed` keyword of the compress entries (zs_deflate_batch_primed; pigz's construction): the
    pieces between the positions of flush_at / flush_every are compressed in parallel, each primed with
    the 32 KiB in front of it, and the output is one ordinary stream at nearly the single-stream ratio.
    Without positions it is an error, and so it is with bgzf; with zdict, a strategy or window_bits /
    mem_level it is refused as flush points are (compress_flush).  Returns whether the call is primed."""
    if not primed:
        return False
    if bgzf is not None and bgzf is not False:
        raise ValueError("primed with bgzf is not built")
    if flush_at is None and flush_every is None:
        raise ValueError("primed needs flush_at or flush_every")
    return True


BGZF_BLOCK = 65280  # ZS_BGZF_BLOCK in zs_gpu.h: the input of one BGZF block at most


def compress_bgzf(bgzf, fmt="gzip", zdict=None, strategy=0, window_bits=None, mem_level=8, flush_at=None,
                  flush_every=None) -> Optional[int]:
    """The `bgzf` keyword of the compress entries (zs_deflate_batch_bgzf; SAM specification 4.1): True for
    blocks of 65,280 input bytes, or the block's bytes.  Returns block_bytes as the C entries take it
    (0 = 65,280), or None for a call without the keyword.  BGZF is a gzip notion and is not built with a
    preset dictionary, a strategy, window_bits / mem_level or flush points (ValueError); a block size out
    of range is left to the engine, which refuses it."""
    if bgzf is None or bgzf is False:
        return None
    if fmt != "gzip":
        raise ValueError('bgzf needs fmt="gzip"')
    if zdict is not None:
        raise ValueError("bgzf with a preset dictionary is not built")
    if strategy:
        raise ValueError("bgzf with strategy %d is not built" % strategy)
    if not _params_default(window_bits, mem_level):
        raise ValueError("bgzf with window_bits / mem_level is not built")
    if flush_at is not None or flush_every is not None:
        raise ValueError("bgzf with flush points is not built")
    if bgzf is True:
        return 0
    if not isinstance(bgzf, int) or bgzf <= 0 or bgzf >= 1 << 32:
        raise ValueError("bgzf is True or the block's bytes")
    return bgzf


def _flush_arrays(per):
    """(flush_first, flush_pos) ctypes arrays of compress_flush's position lists"""
    first, pos = [0], []
    for ps in per:
        pos.extend(ps)
        first.append(len(pos))
    return _arr(ctypes.c_uint64, first), _arr(ctypes.c_uint32, pos)


def _params_default(window_bits, mem_level) -> bool:
    return window_bits in (None, 15) and mem_level == 8


def stream_error_text(status: int, phase: int) -> str:
    if phase == PHASE_INIT:
        return "init failed: %d" % status
    if phase == PHASE_FINISH:
        return "finalization error: %d" % status
    return "process error: %d" % status


_lib = None
_P = ctypes.c_void_p
_U64P = ctypes.POINTER(ctypes.c_uint64)
_U32P = ctypes.POINTER(ctypes.c_uint32)
_I32P = ctypes.POINTER(ctypes.c_int32)


def lib():
    """Load libzsgpu.so (raises ZsUnavailable when it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ZsUnavailable("libzsgpu.so not built: run `make -C zlib-streams-ts_amd/csrc` (or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    L.zs_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(_P)]
    L.zs_ctx_destroy.argtypes = [_P]
    L.zs_last_error.restype = ctypes.c_char_p
    L.zs_version.restype = ctypes.c_char_p
    L.zs_deflate_bound.restype = ctypes.c_uint64
    L.zs_deflate_bound.argtypes = [ctypes.c_uint64, ctypes.c_int]
    L.zs_deflate_batch_device.argtypes = [_P, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, _P, _U64P, _U32P, _P, _U64P,
                                          _U32P, _P, _P, _P]
    L.zs_deflate_batch.argtypes = [_P, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, _U64P, _U32P,
                                   _P, _U64P, _U32P, _I32P, _U32P]
    L.zs_deflate_batch_ex.argtypes = L.zs_deflate_batch.argtypes + [_U32P]
    L.zs_deflate_batch_device_ex.argtypes = [_P, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, _P, _U64P, _U32P, _P,
                                             _U64P, _U32P, _P, _P, _P, _P]
    _inf_host = [ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, _U64P, _U32P]
    _inf_res = [_I32P, _I32P, _I32P, _U32P, _U32P, _U32P]
    L.zs_inflate_batch_ex.argtypes = [_P] + _inf_host + [_P, _U64P, _U32P] + _inf_res
    L.zs_inflate_batch_auto.argtypes = [_P] + _inf_host + [ctypes.POINTER(_P), _U64P] + _inf_res
    _dict = [ctypes.c_char_p, _U64P, _U32P]
    if hasattr(L, "zs_inflate_batch_dict"):  # (ZS_LIB may name an older build)
        L.zs_inflate_batch_dict.argtypes = L.zs_inflate_batch_ex.argtypes + _dict
        L.zs_inflate_batch_dict_auto.argtypes = L.zs_inflate_batch_auto.argtypes + _dict
        L.zs_inflate_batch_dict_device.argtypes = [_P, ctypes.c_int, ctypes.c_uint32, _P, _U64P, _U32P, _P, _U64P,
                                                   _U32P, _P, _P, _P, _P, _P, _P, _P, _P, _U64P, _U32P]
    if hasattr(L, "zs_deflate_batch_dict"):
        L.zs_deflate_bound_dict.restype = ctypes.c_uint64
        L.zs_deflate_bound_dict.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64]
        L.zs_deflate_batch_dict.argtypes = L.zs_deflate_batch_ex.argtypes + _dict
        L.zs_deflate_batch_dict_device.argtypes = L.zs_deflate_batch_device_ex.argtypes + [_P, _U64P, _U32P]
    if hasattr(L, "zs_deflate_batch_strategy"):  # `strategy` behind `level`
        _with = lambda a: a[:2] + [ctypes.c_int] + a[2:]
        L.zs_deflate_batch_strategy.argtypes = _with(L.zs_deflate_batch_ex.argtypes)
        L.zs_deflate_batch_strategy_device.argtypes = _with(L.zs_deflate_batch_device_ex.argtypes)
        L.zs_pool_deflate_batch_strategy.argtypes = _with(L.zs_deflate_batch_ex.argtypes)
    if hasattr(L, "zs_deflate_batch_params"):  # `mem_level` behind `wbits`
        _withm = lambda a: a[:3] + [ctypes.c_int] + a[3:]
        L.zs_deflate_batch_params.argtypes = _withm(L.zs_deflate_batch_ex.argtypes)
        L.zs_deflate_batch_params_device.argtypes = _withm(L.zs_deflate_batch_device_ex.argtypes)
        L.zs_pool_deflate_batch_params.argtypes = _withm(L.zs_deflate_batch_ex.argtypes)
        L.zs_deflate_bound_params.restype = ctypes.c_uint64
        L.zs_deflate_bound_params.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    if hasattr(L, "zs_deflate_batch_flush"):  # `flush`, flush_first, flush_pos behind the counterpart's arguments
        _fl = [ctypes.c_int, _U64P, _U32P]
        L.zs_deflate_batch_flush.argtypes = L.zs_deflate_batch_ex.argtypes + _fl
        L.zs_deflate_batch_flush_device.argtypes = L.zs_deflate_batch_device_ex.argtypes + _fl
        L.zs_pool_deflate_batch_flush.argtypes = L.zs_deflate_batch_ex.argtypes + _fl
        L.zs_deflate_bound_flush.restype = ctypes.c_uint64
        L.zs_deflate_bound_flush.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64]
    if hasattr(L, "zs_deflate_batch_primed"):  # flush_first, flush_pos behind the counterpart's arguments
        _pr = [_U64P, _U32P]
        L.zs_deflate_batch_primed.argtypes = L.zs_deflate_batch_ex.argtypes + _pr
        L.zs_deflate_batch_primed_device.argtypes = L.zs_deflate_batch_device_ex.argtypes + _pr
        L.zs_pool_deflate_batch_primed.argtypes = L.zs_deflate_batch_ex.argtypes + _pr
    if hasattr(L, "zs_deflate_batch_bgzf"):  # no wbits; block_bytes behind the counterpart's arguments
        _nowb = lambda a: a[:2] + a[3:] + [ctypes.c_uint32]
        L.zs_deflate_batch_bgzf.argtypes = _nowb(L.zs_deflate_batch_ex.argtypes)
        L.zs_deflate_batch_bgzf_device.argtypes = _nowb(L.zs_deflate_batch_device_ex.argtypes)
        L.zs_pool_deflate_batch_bgzf.argtypes = _nowb(L.zs_deflate_batch_ex.argtypes)
        L.zs_deflate_bound_bgzf.restype = ctypes.c_uint64
        L.zs_deflate_bound_bgzf.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
        L.zs_last_bgzf_blocks.restype = ctypes.c_uint64
        L.zs_last_bgzf_blocks.argtypes = [_P, _U64P, _U32P, _U32P, ctypes.c_uint64]
    if hasattr(L, "zs_inflate_batch_restart"):  # restart_first, restart_in, restart_out behind the counterpart's arguments
        _rs = [_U64P, _U32P, _U32P]
        L.zs_inflate_batch_restart.argtypes = L.zs_inflate_batch_ex.argtypes + _rs
        L.zs_pool_inflate_batch_restart.argtypes = L.zs_inflate_batch_ex.argtypes + _rs
        L.zs_inflate_batch_restart_device.argtypes = [_P, ctypes.c_int, ctypes.c_uint32, _P, _U64P, _U32P, _P, _U64P,
                                                      _U32P, _P, _P, _P, _P, _P, _P, _P] + _rs
        L.zs_wrapper_header_len.restype = ctypes.c_uint32
        L.zs_wrapper_header_len.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint32]
        L.zs_last_flush_index.restype = ctypes.c_uint64
        L.zs_last_flush_index.argtypes = [_P, _U32P, ctypes.c_uint64]
    if hasattr(L, "zs_inflate_batch_sync"):  # exactly the counterparts' arguments: the points are found
        L.zs_inflate_batch_sync.argtypes = L.zs_inflate_batch_ex.argtypes
        L.zs_pool_inflate_batch_sync.argtypes = L.zs_inflate_batch_ex.argtypes
        L.zs_inflate_batch_sync_device.argtypes = [_P, ctypes.c_int, ctypes.c_uint32, _P, _U64P, _U32P, _P, _U64P, _U32P,
                                                   _P, _P, _P, _P, _P, _P, _P]
        L.zs_last_restart_points.restype = ctypes.c_uint64
        L.zs_last_restart_points.argtypes = [_P, _U64P, _U32P, _U32P, ctypes.c_uint64]
    if hasattr(L, "zs_inflate_batch_members"):  # exactly the counterparts' arguments: the members are found
        L.zs_inflate_batch_members.argtypes = L.zs_inflate_batch_ex.argtypes
        L.zs_pool_inflate_batch_members.argtypes = L.zs_inflate_batch_ex.argtypes
        L.zs_inflate_batch_members_device.argtypes = L.zs_inflate_batch_sync_device.argtypes
        L.zs_last_members.restype = ctypes.c_uint64
        L.zs_last_members.argtypes = [_P, _U64P, _U32P, _U32P, ctypes.c_uint64]
    if hasattr(L, "zs_inflate_batch_bgzf"):  # ... the members' arguments: BGZF blocks are sized from their headers
        L.zs_inflate_batch_bgzf.argtypes = L.zs_inflate_batch_ex.argtypes
        L.zs_pool_inflate_batch_bgzf.argtypes = L.zs_inflate_batch_ex.argtypes
        L.zs_inflate_batch_bgzf_device.argtypes = L.zs_inflate_batch_sync_device.argtypes
        L.zs_last_bgzf_trusted.restype = ctypes.c_uint64
        L.zs_last_bgzf_trusted.argtypes = [_P]
        L.zs_bgzf_out_len.argtypes = [ctypes.c_char_p, ctypes.c_uint32, _U64P]
    if hasattr(L, "zs_inflate_batch_bgzf_range"):  # ... the _bgzf arguments, two arrays of virtual offsets behind in_len
        _rng = lambda a: a[:6] + [_U64P, _U64P] + a[6:]
        L.zs_inflate_batch_bgzf_range.argtypes = _rng(L.zs_inflate_batch_ex.argtypes)
        L.zs_pool_inflate_batch_bgzf_range.argtypes = _rng(L.zs_inflate_batch_ex.argtypes)
        L.zs_inflate_batch_bgzf_range_device.argtypes = _rng(L.zs_inflate_batch_sync_device.argtypes)
        L.zs_bgzf_range_out_len.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, _U64P]
        L.zs_bgzf_voffset.argtypes = [_U32P, _U32P, ctypes.c_uint64, ctypes.c_uint64, _U64P]
    L.zs_free.argtypes = [_P]
    L.zs_pool_create.argtypes = [ctypes.c_uint64, ctypes.POINTER(_P)]
    L.zs_pool_create_list.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(_P)]
    L.zs_pool_destroy.argtypes = [_P]
    L.zs_pool_size.argtypes = [_P]
    L.zs_pool_device.argtypes = [_P, ctypes.c_int]
    L.zs_pool_deflate_batch.argtypes = L.zs_deflate_batch_ex.argtypes
    L.zs_pool_inflate_batch.argtypes = L.zs_inflate_batch_ex.argtypes
    L.zs_pool_inflate_batch_auto.argtypes = L.zs_inflate_batch_auto.argtypes
    if hasattr(L, "zs_pool_inflate_batch_dict"):
        L.zs_pool_inflate_batch_dict.argtypes = L.zs_inflate_batch_dict.argtypes
        L.zs_pool_inflate_batch_dict_auto.argtypes = L.zs_inflate_batch_dict_auto.argtypes
    if hasattr(L, "zs_pool_deflate_batch_dict"):
        L.zs_pool_deflate_batch_dict.argtypes = L.zs_deflate_batch_dict.argtypes
    if hasattr(L, "zs_inflate_batch"):
        L.zs_inflate_batch.argtypes = [_P, ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, _U64P, _U32P, _P, _U64P,
                                       _U32P, _I32P, _I32P, _I32P, _U32P, _U32P]
        L.zs_inflate_batch_device.argtypes = [_P, ctypes.c_int, ctypes.c_uint32, _P, _U64P, _U32P, _P, _U64P, _U32P,
                                              _P, _P, _P, _P, _P, _P]
        L.zs_inflate_message.restype = ctypes.c_char_p
        L.zs_inflate_message.argtypes = [ctypes.c_int32]
    L.zs_crc32_batch_device.argtypes = [_P, ctypes.c_uint32, _P, _U64P, _U32P, _U32P, _P, _P]
    L.zs_adler32_batch_device.argtypes = [_P, ctypes.c_uint32, _P, _U64P, _U32P, _U32P, _P, _P]
    L.zs_crc32_batch.argtypes = [_P, ctypes.c_uint32, ctypes.c_char_p, _U64P, _U32P, _U32P, _U32P]
    L.zs_adler32_batch.argtypes = [_P, ctypes.c_uint32, ctypes.c_char_p, _U64P, _U32P, _U32P, _U32P]
    if hasattr(L, "zs_crc32_combine"):
        for fn in (L.zs_crc32_combine, L.zs_adler32_combine):
            fn.restype = ctypes.c_uint32
            fn.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
        L.zs_last_checksum_parts.restype = ctypes.c_uint32
        L.zs_last_checksum_parts.argtypes = [_P]
    if hasattr(L, "zs_last_host_chunks"):
        L.zs_last_host_chunks.restype = ctypes.c_uint32
        L.zs_last_host_chunks.argtypes = [_P]
    L.zs_last_batch_ms.restype = ctypes.c_double
    L.zs_last_batch_ms.argtypes = [_P]
    L.zs_last_inflate_lane_count.restype = ctypes.c_uint32
    L.zs_last_inflate_lane_count.argtypes = [_P]
    L.zs_last_inflate_seg_count.restype = ctypes.c_uint32
    L.zs_last_inflate_seg_count.argtypes = [_P]
    L.zs_last_phase_ms.restype = ctypes.c_double
    L.zs_last_phase_ms.argtypes = [_P, ctypes.c_char_p]
    L.zs_set_timing.argtypes = [_P, ctypes.c_int]
    L.zs_corpus.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P, ctypes.c_int]
    L.zs_selftest.argtypes = [_P, _U64P]
    L.zs_set_option.argtypes = [_P, ctypes.c_char_p, ctypes.c_int]
    L.zs_debug_fetch.restype = ctypes.c_uint64
    L.zs_debug_fetch.argtypes = [_P, ctypes.c_int, ctypes.c_uint32, _P, ctypes.c_uint64]
    _lib = L
    return L


def build_id() -> str:
    """Identity of the engine build: sha256 (16 hex) over the sources libzsgpu.so
    is compiled from (csrc/*, include/zs_gpu.h).  Committed rocprofv3 summaries
    carry it ("_build_id"); bench.py uses a summary's traffic / counters only
    for the build that produced them."""
    import hashlib

    h = hashlib.sha256()
    csrc = os.path.join(os.path.dirname(_HERE), "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".cpp", ".h")) or f == "Makefile")
    for f in files + ["../../include/zs_gpu.h"]:
        h.update(f.encode() + b"\0")
        with open(os.path.join(csrc, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _arr(ctype, values):
    a = (ctype * max(1, len(values)))(*values)
    return a


def deflate_bound(n: int, fmt: str = "deflate-raw", dict_len: int = 0, n_flush: int = 0, bgzf=None) -> int:
    """deflateBound (deflate.ts:615-674) for a fresh stream, memLevel 8; dict_len: the
    length of its preset dictionary (zs_deflate_bound_dict: DICTID, deflate.ts:633);
    n_flush: its Z_FULL_FLUSH points (zs_deflate_bound_flush: 12 bytes each);
    bgzf=True or the block's bytes: its BGZF file (zs_deflate_bound_bgzf; fmt "gzip")."""
    block = compress_bgzf(bgzf, fmt, b"" if dict_len else None, flush_every=n_flush or None)
    if block is not None:
        if block > BGZF_BLOCK:
            raise ValueError("invalid BGZF block size")
        return int(lib().zs_deflate_bound_bgzf(n, block))
    if n_flush:
        if dict_len:
            raise ValueError("flush points with a preset dictionary are not built")
        return int(lib().zs_deflate_bound_flush(n, compress_wbits(fmt), n_flush))
    if dict_len:
        return int(lib().zs_deflate_bound_dict(n, compress_wbits(fmt), dict_len))
    return int(lib().zs_deflate_bound(n, compress_wbits(fmt)))


def deflate_capacity(n: int, fmt: str = "deflate-raw", dict_len: int = 0) -> int:
    """deflate_bound rounded up to the engine's 4-byte output granularity."""
    return (deflate_bound(n, fmt, dict_len) + 3) & ~3


def wrapper_header_len(data: bytes, fmt: str = "gzip") -> int:
    """zs_wrapper_header_len: the length of the wrapper's header in front of the deflate data -- 0 for
    "deflate-raw", 2 for "deflate", for "gzip" the parsed length (10 plus FEXTRA / FNAME / FCOMMENT /
    FHCRC), or 0 when that header is malformed or does not fit.  Host arithmetic, no GPU."""
    data = bytes(data)
    return int(lib().zs_wrapper_header_len(decompress_wbits(fmt), data, len(data)))


def decompress_scan(restart, out_caps, zdict=None) -> bool:
    """restart="scan": the entry finds the points itself (zs_inflate_batch_sync*).  The capacities must
    be given and dictionaries are not built with it: ValueError, before any call."""
    if not (isinstance(restart, str) and restart == "scan"):
        return False
    if out_caps is None:
        raise ValueError("restart points need out_caps (the unbounded output is not built with them)")
    if zdict is not None:
        raise ValueError("restart points with a preset dictionary are not built")
    return True


def decompress_members(members, fmt, out_caps, zdict=None, restart=None):
    """members=True: every member of a multi-member gzip file is decoded and the outputs are
    concatenated (zs_inflate_batch_members*).  gzip only, the capacities must be given, and neither
    dictionaries nor restart points are built with it: ValueError.  members="bgzf": the same, with BGZF
    blocks sized from their headers (zs_inflate_batch_bgzf*); the host entries size the output themselves
    when out_caps is None (bgzf_out_caps).  Returns False, True or "bgzf"."""
    if not members:
        return False
    if isinstance(members, str):
        if members != "bgzf":
            raise ValueError("members must be True, False or \"bgzf\"")
        if out_caps is None:
            out_caps = ()  # (sized from the headers)
    else:
        members = True
    if fmt != "gzip":
        raise ValueError("members are a gzip notion (fmt must be \"gzip\")")
    if out_caps is None:
        raise ValueError("members need out_caps (the unbounded output is not built with them)")
    if zdict is not None:
        raise ValueError("members with a preset dictionary are not built")
    if restart is not None:
        raise ValueError("members with restart points are not built")
    return members


def bgzf_out_len(data) -> Optional[int]:
    """zs_bgzf_out_len: the bytes a BGZF file produces, read from its headers -- the sum of ISIZE over the
    blocks followed from offset 0 -- or None when a member on the way is no BGZF block whose header can be
    trusted.  Host arithmetic, no GPU."""
    data = bytes(data)
    total = ctypes.c_uint64(0)
    return int(total.value) if lib().zs_bgzf_out_len(data, len(data), ctypes.byref(total)) else None


def bgzf_out_caps(inputs) -> List[int]:
    """the capacities members="bgzf" uses when none are given: each stream's bgzf_out_len rounded up to 4"""
    caps = []
    for i, s in enumerate(inputs):
        n = bgzf_out_len(s)
        if n is None:
            raise ValueError("stream %d is not BGZF throughout: give out_caps" % i)
        caps.append((n + 3) & ~3)
    return caps


def bgzf_range_out_len(data, vb: int, ve: int) -> Optional[int]:
    """zs_bgzf_range_out_len: the bytes the range between the virtual offsets vb and ve (coffset << 16 | uoffset)
    of a BGZF file delivers, read from its headers, or None where the offsets do not follow a chain of BGZF
    blocks.  Host arithmetic, no GPU."""
    data = bytes(data)
    total = ctypes.c_uint64(0)
    ok = lib().zs_bgzf_range_out_len(data, len(data), int(vb), int(ve), ctypes.byref(total))
    return int(total.value) if ok else None


def bgzf_voffset(blocks, upos: int, written: bool = False) -> Optional[int]:
    """zs_bgzf_voffset: the virtual offset of uncompressed position upos, from ONE stream's list of pairs: the last
    block that begins at or before upos.  The list is one of last_members() -- (compressed, uncompressed) offsets -- or,
    with written=True, one of last_bgzf_blocks(), whose pairs are the writer's (in_pos, out_pos) and so (uncompressed,
    compressed); its end-of-file block's entry makes the file's last position addressable.  None when upos lies behind
    the last entry or the difference does not fit 16 bits."""
    c, u = (1, 0) if written else (0, 1)
    voff = ctypes.c_uint64(0)
    ok = lib().zs_bgzf_voffset(_arr(ctypes.c_uint32, [b[c] for b in blocks]), _arr(ctypes.c_uint32, [b[u] for b in blocks]),
                               len(blocks), int(upos), ctypes.byref(voff))
    return int(voff.value) if ok else None


def decompress_ranges(ranges, members, n):
    """The `ranges` keyword of the decompress entries: one (vb, ve) pair of virtual offsets per stream
    (zs_inflate_batch_bgzf_range*).  Only with members="bgzf": ValueError.  Returns the two ctypes arrays, or None."""
    if ranges is None:
        return None
    if not (isinstance(members, str) and members == "bgzf"):
        raise ValueError("ranges need members=\"bgzf\"")
    if len(ranges) != n:
        raise ValueError("ranges: one (vb, ve) pair per stream")
    return (_arr(ctypes.c_uint64, [int(r[0]) for r in ranges]), _arr(ctypes.c_uint64, [int(r[1]) for r in ranges]))


def bgzf_range_out_caps(inputs, ranges) -> List[int]:
    """the capacities ranges= uses when none are given: each stream's bgzf_range_out_len rounded up to 4"""
    caps = []
    for i, (s, r) in enumerate(zip(inputs, ranges)):
        n = bgzf_range_out_len(s, r[0], r[1])
        if n is None:
            raise ValueError("stream %d: the virtual offsets do not follow a chain of BGZF blocks: give out_caps" % i)
        caps.append((n + 3) & ~3)
    return caps


def decompress_restart(inputs, fmt, restart, out_caps, zdict=None):
    """The `restart` keyword of the decompress entries: one list per stream (None / empty = none) of
    (in_pos, out_pos) pairs, the stream's restart points WITHOUT its start -- in_pos the offset in the
    stream's input of the first byte behind a Z_FULL_FLUSH marker, out_pos the uncompressed bytes before
    it (zs_inflate_batch_restart; inflateSync, inflate.ts:1267-1337).  The start, (the wrapper's header
    length, 0), is prepended here.  Returns the (restart_first, restart_in, restart_out) ctypes arrays.
    The capacities must be given, and dictionaries are not built with restart points: ValueError,
    before any call.  Points the entry refuses are its ZS_STREAM_ERROR."""
    if out_caps is None:
        raise ValueError("restart points need out_caps (the unbounded output is not built with them)")
    if zdict is not None:
        raise ValueError("restart points with a preset dictionary are not built")
    per = list(restart)
    if len(per) != len(inputs):
        raise ValueError("restart: %d point lists for %d inputs" % (len(per), len(inputs)))
    first, rin, rout = [0], [], []
    for data, ps in zip(inputs, per):
        pts = [(wrapper_header_len(data, fmt), 0)]
        for pt in ps or []:
            a, b = pt
            for x in (a, b):
                if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x <= 0xffffffff:
                    raise ValueError("restart: points are pairs of ints in 0 .. 2^32 - 1")
            pts.append((a, b))
        rin.extend(a for a, _ in pts)
        rout.extend(b for _, b in pts)
        first.append(len(rin))
    return _arr(ctypes.c_uint64, first), _arr(ctypes.c_uint32, rin), _arr(ctypes.c_uint32, rout)


def crc32_combine(crc1: int, crc2: int, len2: int) -> int:
    """zs_crc32_combine: the crc32 of A + B from crc32(A), crc32(B) and len(B) (zlib's
    crc32_combine; host arithmetic, no GPU)."""
    return int(lib().zs_crc32_combine(crc1 & 0xffffffff, crc2 & 0xffffffff, len2))


def adler32_combine(adler1: int, adler2: int, len2: int) -> int:
    """zs_adler32_combine: the adler32 of A + B from adler32(A), adler32(B) and len(B)
    (zlib's adler32_combine, for reduced values; host arithmetic, no GPU)."""
    return int(lib().zs_adler32_combine(adler1 & 0xffffffff, adler2 & 0xffffffff, len2))


class Engine:
    """One device context (one per GPU / process)."""

    def __init__(self, device: int = 0):
        L = lib()
        ctx = _P()
        r = L.zs_ctx_create(device, ctypes.byref(ctx))
        if r != 0:
            raise ZsUnavailable("zs_ctx_create(%d) failed: %s" % (device, L.zs_last_error().decode()))
        self._L, self._ctx, self.device = L, ctx, device

    def selftest(self) -> int:
        """Lane-order violations of same-address LDS atomics (0 expected; see selftest.hip)."""
        v = ctypes.c_uint64(0)
        r = self._L.zs_selftest(self._ctx, ctypes.byref(v))
        if r != 0:
            raise ZsError("zs_selftest failed: %s" % self._L.zs_last_error().decode())
        return int(v.value)

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.zs_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._ctx

    def set_option(self, name: str, value: int):
        """zs_set_option: "timing", "inflate_fast", "check_phases", "match_sweep", ...; "checksum_split"
        (bytes, 0 = never) and "checksum_part" (a power of two 1024 .. 1048576): a batch with a
        longer stream computes its data checksums in parts; "host_chunk_min" (input bytes from which a
        host batch of 64 streams or more runs as four chunks, 0 = never) and "host_pack_min" (the floor
        of the packed-output buffers' first size) (see zs_gpu.h)."""
        if self._L.zs_set_option(self._ctx, name.encode(), int(value)) != 0:
            raise ZsError(self._L.zs_last_error().decode())

    def debug_fetch(self, what: int, stream: int, nbytes: int) -> bytes:
        """zs_debug_fetch: an intermediate array of `stream` from the last deflate batch
        (0 links/members u16, 1 match table u32x2 per position, 2 symbols, ...)."""
        buf = ctypes.create_string_buffer(max(1, nbytes))
        k = self._L.zs_debug_fetch(self._ctx, what, stream, buf, nbytes)
        return buf.raw[:k]

    def bucket_members(self, stream: int) -> bytes:
        """the sweep route's members (u16 each) of `stream`'s first window in the last deflate batch"""
        return self.debug_fetch(7, stream, 2 * 65535)

    def set_timing(self, on: bool):
        self._L.zs_set_timing(self._ctx, 1 if on else 0)

    def last_lane_count(self) -> int:
        """members of the last inflate batch decoded by the lane path"""
        return self._L.zs_last_inflate_lane_count(self._ctx)

    def last_seg_count(self) -> int:
        """members of the last inflate batch the segmented decode finished (inflate_seg.hip)"""
        return self._L.zs_last_inflate_seg_count(self._ctx)

    def last_checksum_parts(self) -> int:
        """parts of the last batch call's data checksum (0: one wave per stream; zs_last_checksum_parts)"""
        return self._L.zs_last_checksum_parts(self._ctx)

    def last_host_chunks(self) -> int:
        """chunks the last host-buffer compress / decompress call ran as: 1 or 4 (options "host_chunk_min",
        "host_pack_min"); 0 after a device call (zs_last_host_chunks)"""
        return self._L.zs_last_host_chunks(self._ctx)

    def last_ms(self, phase: Optional[str] = None) -> float:
        if phase is None:
            return self._L.zs_last_batch_ms(self._ctx)
        return self._L.zs_last_phase_ms(self._ctx, phase.encode())

    def _check(self, r: int, what: str):
        if r != 0:
            msg = self._L.zs_last_error().decode()
            if r == Z_STREAM_ERROR:
                raise ZsError("init failed: %d" % r, r, PHASE_INIT, msg)
            raise ZsUnavailable("%s failed (%d): %s" % (what, r, msg))

    # ---------------------------------------------------------- host buffers
    def compress_batch_raw(self, inputs: Sequence[bytes], fmt: str = "deflate-raw", level: int = -1, zdict=None,
                           strategy: int = 0, window_bits=None, mem_level=8, flush_at=None,
                           flush_every=None, bgzf=None, primed=False) -> List[Tuple[int, bytes]]:
        """Returns [(status, bytes)] -- status Z_STREAM_END on success.
        zdict: a preset dictionary for every input (bytes), or one per input (a
        list; None = none) -- "deflate-raw" and "deflate" only, levels 1..9
        (zs_deflate_batch_dict: deflateSetDictionary, deflate.ts:367-424).
        strategy: Z_DEFAULT_STRATEGY .. Z_FIXED (zs_deflate_batch_strategy; not with zdict).
        window_bits (8..15, None = 15), mem_level (1..9): deflateInit2_'s windowBits and memLevel
        (zs_deflate_batch_params; other than 15 / 8 not with zdict or a strategy, levels 1..9).
        flush_at (positions for every stream, or a list per stream), flush_every=N: Z_FULL_FLUSH
        points (zs_deflate_batch_flush; levels 1..9, not with any of the above).
        primed=True with flush_at / flush_every: no flush but primed pieces between the positions, each
        compressed against the 32 KiB in front of it (zs_deflate_batch_primed): one ordinary stream.
        bgzf=True or the block's bytes: BGZF blocks and the end-of-file block (zs_deflate_batch_bgzf;
        fmt "gzip", levels 0..9, not with any of the above)."""
        return [(st, b) for st, b, _ in self.compress_batch_detailed(inputs, fmt, level, zdict, strategy, window_bits,
                                                                     mem_level, flush_at, flush_every, bgzf, primed)]

    def compress_batch_detailed(self, inputs: Sequence[bytes], fmt: str = "deflate-raw", level: int = -1, zdict=None,
                                strategy: int = 0, window_bits=None, mem_level=8, flush_at=None,
                                flush_every=None, bgzf=None, primed=False) -> List[Tuple[int, bytes, int]]:
        """Returns [(status, bytes, check)]: check = the reference's strm.adler after the
        stream (adler32 / crc32 of the input for deflate / gzip, 1 for deflate-raw)."""
        primed = compress_primed(primed, flush_at, flush_every, bgzf)
        block = compress_bgzf(bgzf, fmt, zdict, strategy, window_bits, mem_level, flush_at, flush_every)
        self._bgzf_n = 0
        if block is not None:
            self._flush_counts = None
            self._bgzf_n = len(inputs)
            return _deflate_host_bgzf(self._L, self._L.zs_deflate_batch_bgzf, self._ctx, inputs, level, self._check,
                                      block)
        compress_strategy(strategy, zdict)
        code = compress_params(fmt, window_bits, mem_level, zdict, strategy)
        per = compress_flush([len(b) for b in inputs], flush_at, flush_every, zdict, strategy, window_bits, mem_level)
        self._flush_counts = None
        if per is not None:
            self._flush_counts = [len(ps) for ps in per]
            fn = self._L.zs_deflate_batch_primed if primed else self._L.zs_deflate_batch_flush
            return _deflate_host(self._L, fn, self._ctx, inputs, fmt, level, self._check, flush=per, primed=primed)
        if not _params_default(window_bits, mem_level):
            return _deflate_host(self._L, self._L.zs_deflate_batch_params, self._ctx, inputs, fmt, level, self._check,
                                 params=(code, mem_level))
        if compress_strategy(strategy, zdict):
            return _deflate_host(self._L, self._L.zs_deflate_batch_strategy, self._ctx, inputs, fmt, level,
                                 self._check, strategy=strategy)
        if zdict is not None:
            return _deflate_host(self._L, self._L.zs_deflate_batch_dict, self._ctx, inputs, fmt, level, self._check,
                                 _dict_layout(zdict, len(inputs)))
        return _deflate_host(self._L, self._L.zs_deflate_batch_ex, self._ctx, inputs, fmt, level, self._check)

    def compress_batch(self, inputs: Sequence[bytes], fmt: str = "deflate-raw", level: int = -1, zdict=None,
                       strategy: int = 0, window_bits=None, mem_level=8, flush_at=None, flush_every=None,
                       bgzf=None, primed=False) -> List[bytes]:
        return _ok_or_raise_c(self.compress_batch_raw(inputs, fmt, level, zdict, strategy, window_bits, mem_level,
                                                      flush_at, flush_every, bgzf, primed))

    def decompress_batch_raw(self, inputs: Sequence[bytes], fmt: str = "deflate-raw",
                             out_caps: Optional[Sequence[int]] = None, zdict=None, restart=None, members=False,
                             ranges=None):
        """Returns [(status, phase, msg, bytes, consumed)].  out_caps None: unbounded
        output, as DecompressionStream (zs_inflate_batch_auto); else per-stream caps.
        zdict: a preset dictionary for every input (bytes), or one per input (a
        list; None = none) -- "deflate-raw" and "deflate" only (zs_inflate_batch_dict*).
        restart: one list per input of (in_pos, out_pos) restart points (decompress_restart;
        zs_inflate_batch_restart: the segments decode in parallel, zlib semantics; needs out_caps), or
        "scan": the points are found from the bytes (zs_inflate_batch_sync; last_restart_points()).
        members=True: every member of multi-member gzip inputs, concatenated (decompress_members;
        zs_inflate_batch_members; last_members()).  members="bgzf": the same for BGZF files, the blocks
        sized from their headers (zs_inflate_batch_bgzf; last_bgzf_trusted()); out_caps None: sized from
        the headers too (bgzf_out_caps; ValueError for a stream that is not BGZF throughout).
        ranges=[(vb, ve), ...] with members="bgzf": per stream, the bytes between two virtual offsets
        (zs_inflate_batch_bgzf_range; inputs that are the same object are laid out once, so many ranges may
        name one file); out_caps None: sized with bgzf_range_out_len."""
        return [r[:5] for r in self.decompress_batch_detailed(inputs, fmt, out_caps, zdict, restart, members, ranges)]

    def decompress_batch_detailed(self, inputs: Sequence[bytes], fmt: str = "deflate-raw",
                                  out_caps: Optional[Sequence[int]] = None, zdict=None, restart=None, members=False,
                                  ranges=None):
        """Returns [(status, phase, msg, bytes, consumed, check)]."""
        L = self._L
        rng = decompress_ranges(ranges, members, len(inputs))
        mode = decompress_members(members, fmt, out_caps, zdict, restart)
        if rng is not None:
            caps = bgzf_range_out_caps(inputs, ranges) if out_caps is None else out_caps
            self._members_n = 0
            return _inflate_host(L, L.zs_inflate_batch_bgzf_range, self._ctx, inputs, fmt, caps, self._check, ranges=rng)
        if mode == "bgzf":
            caps = bgzf_out_caps(inputs) if out_caps is None else out_caps
            res = _inflate_host(L, L.zs_inflate_batch_bgzf, self._ctx, inputs, fmt, caps, self._check)
            self._members_n = len(inputs)
            return res
        if mode:
            res = _inflate_host(L, L.zs_inflate_batch_members, self._ctx, inputs, fmt, out_caps, self._check)
            self._members_n = len(inputs)  # (a refused call leaves the context's record, and this count, alone)
            return res
        if decompress_scan(restart, out_caps, zdict):
            res = _inflate_host(L, L.zs_inflate_batch_sync, self._ctx, inputs, fmt, out_caps, self._check)
            self._sync_n = len(inputs)  # (a refused call leaves the context's record, and this count, alone)
            return res
        if restart is not None:
            rs = decompress_restart(inputs, fmt, restart, out_caps, zdict)
            return _inflate_host(L, L.zs_inflate_batch_restart, self._ctx, inputs, fmt, out_caps, self._check, rs)
        if zdict is not None:
            d = _dict_layout(zdict, len(inputs))
            if out_caps is None:
                return _inflate_host_auto(L, L.zs_inflate_batch_dict_auto, self._ctx, inputs, fmt, self._check, d)
            return _inflate_host(L, L.zs_inflate_batch_dict, self._ctx, inputs, fmt, out_caps, self._check, d)
        if out_caps is None:
            return _inflate_host_auto(L, L.zs_inflate_batch_auto, self._ctx, inputs, fmt, self._check)
        return _inflate_host(L, L.zs_inflate_batch_ex, self._ctx, inputs, fmt, out_caps, self._check)

    def decompress_batch(self, inputs: Sequence[bytes], fmt: str = "deflate-raw",
                         out_caps: Optional[Sequence[int]] = None, zdict=None, restart=None, members=False,
                         ranges=None) -> List[bytes]:
        return _ok_or_raise_d(self.decompress_batch_raw(inputs, fmt, out_caps, zdict, restart, members, ranges))

    def last_members(self) -> List[List[tuple]]:
        """zs_last_members: the members the last members=True call on this engine decoded, one list per
        stream of (in_pos, out_pos), member 0 = (0, 0) included.  [] when the last decompress call was
        no members call."""
        n = getattr(self, "_members_n", 0)
        if not n:
            return []
        first = (ctypes.c_uint64 * (n + 1))()
        total = int(self._L.zs_last_members(self._ctx, first, None, None, 0))
        if total == 0:
            return []
        min_, mout = (ctypes.c_uint32 * total)(), (ctypes.c_uint32 * total)()
        if int(self._L.zs_last_members(self._ctx, first, min_, mout, total)) != total or first[n] != total:
            raise ZsError("zs_last_members: the count changed between two queries")
        return [[(int(min_[k]), int(mout[k])) for k in range(first[i], first[i + 1])] for i in range(n)]

    def last_bgzf_trusted(self) -> int:
        """zs_last_bgzf_trusted: the planned members of the last members="bgzf" call on this engine whose
        size came from their header; 0 after any other decompress call."""
        return int(self._L.zs_last_bgzf_trusted(self._ctx))

    def last_bgzf_blocks(self) -> List[List[tuple]]:
        """zs_last_bgzf_blocks: the blocks of the last bgzf= compress call on this engine, one list per
        stream of (in_pos, out_pos) -- the offset of the block's first input byte and of its first byte
        in the stream's output -- the end-of-file block's (len(input), len(output) - 28) last: a .gzi
        index plus the end.  [] when the last compress call was no bgzf call.  Synchronises."""
        n = getattr(self, "_bgzf_n", 0)
        if not n:
            return []
        first = (ctypes.c_uint64 * (n + 1))()
        total = int(self._L.zs_last_bgzf_blocks(self._ctx, first, None, None, 0))
        if total == 0:
            return []
        bin_, bout = (ctypes.c_uint32 * total)(), (ctypes.c_uint32 * total)()
        if int(self._L.zs_last_bgzf_blocks(self._ctx, first, bin_, bout, total)) != total or first[n] != total:
            raise ZsError("zs_last_bgzf_blocks: the count changed between two queries")
        return [[(int(bin_[k]), int(bout[k])) for k in range(first[i], first[i + 1])] for i in range(n)]

    def last_restart_points(self) -> List[List[tuple]]:
        """zs_last_restart_points: the points the last restart="scan" call on this engine found, one
        list per stream of (in_pos, out_pos) WITHOUT the start -- the shape `restart=` takes, so a
        caller can keep them as an index.  [] when the last decompress call was no scan call."""
        n = getattr(self, "_sync_n", 0)
        if not n:
            return []
        first = (ctypes.c_uint64 * (n + 1))()
        total = int(self._L.zs_last_restart_points(self._ctx, first, None, None, 0))
        if total == 0:
            return []
        rin, rout = (ctypes.c_uint32 * total)(), (ctypes.c_uint32 * total)()
        if int(self._L.zs_last_restart_points(self._ctx, first, rin, rout, total)) != total or first[n] != total:
            raise ZsError("zs_last_restart_points: the count changed between two queries")
        return [[(int(rin[k]), int(rout[k])) for k in range(first[i] + 1, first[i + 1])] for i in range(n)]

    def last_flush_index(self) -> List[List[int]]:
        """zs_last_flush_index: for the last compress call with flush points on this engine
        (compress_batch*(..., flush_at / flush_every) or compress_device), one list per stream of the
        offsets in its output of the byte behind each marker: the in_pos of the restart points whose
        out_pos are the flush positions.  Synchronises."""
        per = getattr(self, "_flush_counts", None)
        if not per:
            return []
        total = sum(per)
        buf = (ctypes.c_uint32 * max(1, total))()
        k = int(self._L.zs_last_flush_index(self._ctx, buf, total))
        if k != total:
            raise ZsError("zs_last_flush_index: %d points, %d expected" % (k, total))
        out, at = [], 0
        for c in per:
            out.append(list(buf[at: at + c]))
            at += c
        return out

    # ---------------------------------------------------- device-resident
    def compress_device(self, level: int, fmt: str, n: int, d_in: int, in_off, in_len, d_out: int, out_off, out_cap,
                        d_status: int, d_out_len: int, hip_stream: int = 0, d_check: int = 0, d_dict: int = 0,
                        dict_off=None, dict_len=None, strategy: int = 0, window_bits=None, mem_level=8, flush_at=None,
                        flush_every=None, bgzf=None, primed=False):
        """Device pointers (ints) + host layout arrays (ctypes arrays).
        primed=True with flush_at / flush_every: primed pieces (zs_deflate_batch_primed_device).
        bgzf=True or the block's bytes: BGZF (zs_deflate_batch_bgzf_device; fmt "gzip", not with the others).
        flush_at / flush_every: Z_FULL_FLUSH points (zs_deflate_batch_flush_device; not with the others).
        d_dict / dict_off / dict_len: preset dictionaries (zs_deflate_batch_dict_device:
        device bytes, host ctypes arrays of per-stream offsets and lengths, 0 = none).
        strategy: zs_deflate_batch_strategy_device (not with dictionaries).
        window_bits / mem_level: zs_deflate_batch_params_device (other than 15 / 8 not with either)."""
        primed = compress_primed(primed, flush_at, flush_every, bgzf)
        block = compress_bgzf(bgzf, fmt, dict_off, strategy, window_bits, mem_level, flush_at, flush_every)
        self._bgzf_n = 0
        if block is not None:
            self._flush_counts = None
            r = self._L.zs_deflate_batch_bgzf_device(self._ctx, compress_level(level), n, _P(d_in), in_off, in_len,
                                                     _P(d_out), out_off, out_cap, _P(d_status), _P(d_out_len),
                                                     _P(d_check) if d_check else None,
                                                     _P(hip_stream) if hip_stream else None, block)
            self._check(r, "zs_deflate_batch_bgzf_device")
            self._bgzf_n = n
            return
        compress_strategy(strategy, dict_off)
        code = compress_params(fmt, window_bits, mem_level, dict_off, strategy)
        per = compress_flush([in_len[i] for i in range(n)], flush_at, flush_every, dict_off, strategy, window_bits,
                             mem_level)
        self._flush_counts = None
        if per is not None:
            self._flush_counts = [len(ps) for ps in per]
            first, pos = _flush_arrays(per)
            if primed:
                r = self._L.zs_deflate_batch_primed_device(self._ctx, compress_level(level), compress_wbits(fmt), n,
                                                           _P(d_in), in_off, in_len, _P(d_out), out_off, out_cap,
                                                           _P(d_status), _P(d_out_len), _P(d_check) if d_check else None,
                                                           _P(hip_stream) if hip_stream else None, first, pos)
                self._check(r, "zs_deflate_batch_primed_device")
                return
            r = self._L.zs_deflate_batch_flush_device(self._ctx, compress_level(level), compress_wbits(fmt), n,
                                                      _P(d_in), in_off, in_len, _P(d_out), out_off, out_cap,
                                                      _P(d_status), _P(d_out_len), _P(d_check) if d_check else None,
                                                      _P(hip_stream) if hip_stream else None, Z_FULL_FLUSH, first, pos)
            self._check(r, "zs_deflate_batch_flush_device")
            return
        if not _params_default(window_bits, mem_level):
            r = self._L.zs_deflate_batch_params_device(self._ctx, compress_level(level), code, mem_level, n, _P(d_in),
                                                       in_off, in_len, _P(d_out), out_off, out_cap, _P(d_status),
                                                       _P(d_out_len), _P(d_check) if d_check else None,
                                                       _P(hip_stream) if hip_stream else None)
            self._check(r, "zs_deflate_batch_params_device")
            return
        if compress_strategy(strategy, dict_off):
            r = self._L.zs_deflate_batch_strategy_device(self._ctx, compress_level(level), strategy,
                                                         compress_wbits(fmt), n, _P(d_in), in_off, in_len, _P(d_out),
                                                         out_off, out_cap, _P(d_status), _P(d_out_len),
                                                         _P(d_check) if d_check else None,
                                                         _P(hip_stream) if hip_stream else None)
            self._check(r, "zs_deflate_batch_strategy_device")
            return
        if dict_off is not None:
            r = self._L.zs_deflate_batch_dict_device(self._ctx, compress_level(level), compress_wbits(fmt), n,
                                                     _P(d_in), in_off, in_len, _P(d_out), out_off, out_cap,
                                                     _P(d_status), _P(d_out_len), _P(d_check) if d_check else None,
                                                     _P(hip_stream) if hip_stream else None,
                                                     _P(d_dict) if d_dict else None, dict_off, dict_len)
            self._check(r, "zs_deflate_batch_dict_device")
            return
        r = self._L.zs_deflate_batch_device_ex(self._ctx, compress_level(level), compress_wbits(fmt), n, _P(d_in),
                                               in_off, in_len, _P(d_out), out_off, out_cap, _P(d_status),
                                               _P(d_out_len), _P(d_check) if d_check else None,
                                               _P(hip_stream) if hip_stream else None)
        self._check(r, "zs_deflate_batch_device")

    def decompress_device(self, fmt: str, n: int, d_in: int, in_off, in_len, d_out: int, out_off, out_cap,
                          d_status: int, d_phase: int, d_msg: int, d_out_len: int, d_consumed: int,
                          hip_stream: int = 0, d_dict: int = 0, dict_off=None, dict_len=None, d_check: int = 0,
                          restart=None, headers=None, members=False, ranges=None):
        """d_dict / dict_off / dict_len: preset dictionaries (zs_inflate_batch_dict_device:
        device bytes, host ctypes arrays of per-stream offsets and lengths, 0 = none).
        restart: one list per stream of (in_pos, out_pos) restart points without the start
        (zs_inflate_batch_restart_device); the streams' bytes are on the device, so `headers` gives the
        first bytes of each stream on the host (enough to hold its wrapper's header; not needed for
        "deflate-raw" and "deflate") for the first point.  restart="scan": the points are found from the
        bytes on the device (zs_inflate_batch_sync_device, which waits for hip_stream once in the
        middle); no `headers`.  members=True: every member of multi-member gzip streams
        (zs_inflate_batch_members_device, which waits for hip_stream as the scan call does); members="bgzf":
        BGZF blocks sized from their headers (zs_inflate_batch_bgzf_device); with ranges=[(vb, ve), ...] the
        bytes between two virtual offsets per stream (zs_inflate_batch_bgzf_range_device)."""
        rng = decompress_ranges(ranges, members, n)
        mode = decompress_members(members, fmt, out_cap, None if dict_off is None else dict_off, restart)
        if rng is not None:
            if out_cap is None:
                raise ValueError("members on the device need out_cap")
            r = self._L.zs_inflate_batch_bgzf_range_device(
                self._ctx, decompress_wbits(fmt), n, _P(d_in), in_off, in_len, rng[0], rng[1], _P(d_out), out_off, out_cap,
                _P(d_status), _P(d_phase), _P(d_msg), _P(d_out_len), _P(d_consumed), _P(d_check) if d_check else None,
                _P(hip_stream) if hip_stream else None)
            self._check(r, "zs_inflate_batch_bgzf_range_device")
            self._members_n = 0
            return
        if mode:
            bgzf = mode == "bgzf"  # (the regions are the caller's: out_cap is needed, as with members=True)
            if out_cap is None:
                raise ValueError("members on the device need out_cap")
            fn = self._L.zs_inflate_batch_bgzf_device if bgzf else self._L.zs_inflate_batch_members_device
            r = fn(self._ctx, decompress_wbits(fmt), n, _P(d_in), in_off, in_len, _P(d_out), out_off, out_cap,
                   _P(d_status), _P(d_phase), _P(d_msg), _P(d_out_len), _P(d_consumed),
                   _P(d_check) if d_check else None, _P(hip_stream) if hip_stream else None)
            self._check(r, "zs_inflate_batch_bgzf_device" if bgzf else "zs_inflate_batch_members_device")
            self._members_n = n
            return
        if decompress_scan(restart, out_cap, None if dict_off is None else dict_off):
            r = self._L.zs_inflate_batch_sync_device(self._ctx, decompress_wbits(fmt), n, _P(d_in), in_off, in_len,
                                                     _P(d_out), out_off, out_cap, _P(d_status), _P(d_phase), _P(d_msg),
                                                     _P(d_out_len), _P(d_consumed), _P(d_check) if d_check else None,
                                                     _P(hip_stream) if hip_stream else None)
            self._check(r, "zs_inflate_batch_sync_device")
            self._sync_n = n
            return
        if restart is not None:
            if dict_off is not None:
                raise ValueError("restart points with a preset dictionary are not built")
            if headers is None:
                if fmt == "gzip":
                    raise ValueError("restart points of gzip streams on the device need `headers`")
                headers = [b""] * n
            rs = decompress_restart(headers, fmt, restart, out_cap)
            r = self._L.zs_inflate_batch_restart_device(self._ctx, decompress_wbits(fmt), n, _P(d_in), in_off, in_len,
                                                        _P(d_out), out_off, out_cap, _P(d_status), _P(d_phase),
                                                        _P(d_msg), _P(d_out_len), _P(d_consumed),
                                                        _P(d_check) if d_check else None,
                                                        _P(hip_stream) if hip_stream else None, *rs)
            self._check(r, "zs_inflate_batch_restart_device")
            return
        if dict_off is not None:
            r = self._L.zs_inflate_batch_dict_device(self._ctx, decompress_wbits(fmt), n, _P(d_in), in_off, in_len,
                                                     _P(d_out), out_off, out_cap, _P(d_status), _P(d_phase),
                                                     _P(d_msg), _P(d_out_len), _P(d_consumed),
                                                     _P(d_check) if d_check else None,
                                                     _P(hip_stream) if hip_stream else None,
                                                     _P(d_dict) if d_dict else None, dict_off, dict_len)
            self._check(r, "zs_inflate_batch_dict_device")
            return
        r = self._L.zs_inflate_batch_device(self._ctx, decompress_wbits(fmt), n, _P(d_in), in_off, in_len, _P(d_out),
                                            out_off, out_cap, _P(d_status), _P(d_phase), _P(d_msg), _P(d_out_len),
                                            _P(d_consumed), _P(hip_stream) if hip_stream else None)
        self._check(r, "zs_inflate_batch_device")

    def compress_host(self, level: int, fmt: str, n: int, h_in: int, in_off, in_len, h_out: int, out_off, out_cap,
                      status, out_len, strategy: int = 0, window_bits=None, mem_level=8, bgzf=None):
        """zs_deflate_batch on caller-owned host memory (pointers as ints,
        layout/result arrays as ctypes arrays): the end-to-end host->host path
        (strategy: zs_deflate_batch_strategy; window_bits / mem_level: zs_deflate_batch_params;
        bgzf: zs_deflate_batch_bgzf, fmt "gzip")."""
        block = compress_bgzf(bgzf, fmt, None, strategy, window_bits, mem_level)
        self._bgzf_n = 0
        if block is not None:
            self._flush_counts = None
            r = self._L.zs_deflate_batch_bgzf(self._ctx, compress_level(level), n, ctypes.cast(h_in, ctypes.c_char_p),
                                              in_off, in_len, _P(h_out), out_off, out_cap, status, out_len, None, block)
            self._check(r, "zs_deflate_batch_bgzf")
            self._bgzf_n = n
            return
        compress_strategy(strategy)
        code = compress_params(fmt, window_bits, mem_level, None, strategy)
        if not _params_default(window_bits, mem_level):
            r = self._L.zs_deflate_batch_params(self._ctx, level, code, mem_level, n,
                                                ctypes.cast(h_in, ctypes.c_char_p), in_off, in_len, _P(h_out), out_off,
                                                out_cap, status, out_len, None)
            self._check(r, "zs_deflate_batch_params")
            return
        if compress_strategy(strategy):
            r = self._L.zs_deflate_batch_strategy(self._ctx, level, strategy, compress_wbits(fmt), n,
                                                  ctypes.cast(h_in, ctypes.c_char_p), in_off, in_len, _P(h_out),
                                                  out_off, out_cap, status, out_len, None)
            self._check(r, "zs_deflate_batch_strategy")
            return
        r = self._L.zs_deflate_batch(self._ctx, level, compress_wbits(fmt), n, ctypes.cast(h_in, ctypes.c_char_p),
                                     in_off, in_len, _P(h_out), out_off, out_cap, status, out_len)
        self._check(r, "zs_deflate_batch")

    def decompress_host(self, fmt: str, n: int, h_in: int, in_off, in_len, h_out: int, out_off, out_cap, status,
                        phase, msg, out_len, consumed):
        """zs_inflate_batch on caller-owned host memory (pointers as ints, layout /
        result arrays as ctypes arrays): the end-to-end host->host decode."""
        r = self._L.zs_inflate_batch(self._ctx, decompress_wbits(fmt), n, ctypes.cast(h_in, ctypes.c_char_p), in_off,
                                     in_len, _P(h_out), out_off, out_cap, status, phase, msg, out_len, consumed)
        self._check(r, "zs_inflate_batch")

    def checksum_device(self, kind: str, n: int, d_in: int, in_off, in_len, d_check: int, hip_stream: int = 0,
                        seeds=None):
        """crc32 / adler32 of n device-resident streams (seeds: ctypes u32 array or None)"""
        fn = self._L.zs_crc32_batch_device if kind == "crc32" else self._L.zs_adler32_batch_device
        r = fn(self._ctx, n, _P(d_in), in_off, in_len, seeds, _P(d_check), _P(hip_stream) if hip_stream else None)
        self._check(r, "checksum")

    def checksum(self, kind: str, bufs: Sequence[bytes], seeds: Optional[Sequence[int]] = None) -> List[int]:
        """[crc32(seed, buf)] or [adler32(seed, buf)] per buffer (common/crc32.ts:26,
        common/adler32.ts:4 semantics; seeds None = initial values)."""
        n = len(bufs)
        if n == 0:
            return []
        offs, lens, o = [], [], 0
        for b in bufs:
            offs.append(o)
            lens.append(len(b))
            o += len(b)
        sd = (ctypes.c_uint32 * n)(*[x & 0xffffffff for x in seeds]) if seeds is not None else None
        out = (ctypes.c_uint32 * n)()
        fn = self._L.zs_crc32_batch if kind == "crc32" else self._L.zs_adler32_batch
        r = fn(self._ctx, n, b"".join(bufs), (ctypes.c_uint64 * n)(*offs), (ctypes.c_uint32 * n)(*lens), sd, out)
        self._check(r, "checksum")
        return list(out)

    def crc32(self, bufs: Sequence[bytes], seeds: Optional[Sequence[int]] = None) -> List[int]:
        return self.checksum("crc32", bufs, seeds)

    def adler32(self, bufs: Sequence[bytes], seeds: Optional[Sequence[int]] = None) -> List[int]:
        return self.checksum("adler32", bufs, seeds)


def _layout(inputs):
    offs, lens, o = [], [], 0
    for b in inputs:
        offs.append(o)
        lens.append(len(b))
        o += len(b)
    return b"".join(inputs), offs, lens


def _deflate_host(L, fn, handle, inputs, fmt, level, check, zdict=(), strategy=None, params=None, flush=None,
                  primed=False):
    """params: (the windowBits code, mem_level) for a _params entry (fn), which takes mem_level behind wbits.
    flush: compress_flush's position lists for a _flush entry, which takes them behind `check`; primed: fn
    is a _primed entry, which takes them without the flush argument."""
    n = len(inputs)
    if n == 0:
        return []
    wbits = compress_wbits(fmt) if params is None else params[0]
    blob, offs, lens = _layout(inputs)
    if params is not None:
        lv = compress_level(level)
        caps = [(int(L.zs_deflate_bound_params(len(b), wbits, params[1], 6 if lv == -1 else lv)) + 3) & ~3
                for b in inputs]
    elif flush is not None:
        caps = [(int(L.zs_deflate_bound_flush(len(b), wbits, len(flush[i]))) + 3) & ~3 for i, b in enumerate(inputs)]
        zdict = (() if primed else (Z_FULL_FLUSH,)) + _flush_arrays(flush)  # (the trailing arguments)
    elif zdict:
        caps = [(int(L.zs_deflate_bound_dict(len(b), wbits, zdict[2][i])) + 3) & ~3 for i, b in enumerate(inputs)]
    else:
        caps = [(int(L.zs_deflate_bound(len(b), wbits)) + 3) & ~3 for b in inputs]
    ooffs, oo = [], 0
    for c in caps:
        ooffs.append(oo)
        oo += c
    out = ctypes.create_string_buffer(max(1, oo))
    status, olen, chk = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    lead = (compress_level(level),) if strategy is None else (compress_level(level), strategy)  # (fn: a _strategy entry)
    mid = (wbits,) if params is None else (wbits, params[1])
    r = fn(handle, *lead, *mid, n, blob, _arr(ctypes.c_uint64, offs), _arr(ctypes.c_uint32, lens),
           out, _arr(ctypes.c_uint64, ooffs), _arr(ctypes.c_uint32, caps), status, olen, chk, *zdict)
    check(r, "deflate batch")
    raw = out.raw
    return [(status[i], raw[ooffs[i]: ooffs[i] + olen[i]], chk[i]) for i in range(n)]


def _deflate_host_bgzf(L, fn, handle, inputs, level, check, block):
    """_deflate_host for a _bgzf entry (fn), which takes no wbits and block_bytes behind `check`."""
    n = len(inputs)
    if n == 0:
        return []
    blob, offs, lens = _layout(inputs)
    # (a block size the engine will refuse has no bound: the call is made all the same, for its error)
    caps = [(int(L.zs_deflate_bound_bgzf(len(b), min(block, 0xffffffff))) + 3) & ~3 for b in inputs]
    ooffs, oo = [], 0
    for c in caps:
        ooffs.append(oo)
        oo += c
    out = ctypes.create_string_buffer(max(1, oo))
    status, olen, chk = (ctypes.c_int32 * n)(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    r = fn(handle, compress_level(level), n, blob, _arr(ctypes.c_uint64, offs), _arr(ctypes.c_uint32, lens), out,
           _arr(ctypes.c_uint64, ooffs), _arr(ctypes.c_uint32, caps), status, olen, chk, block)
    check(r, "deflate batch")
    raw = out.raw
    return [(status[i], raw[ooffs[i]: ooffs[i] + olen[i]], chk[i]) for i in range(n)]


def _inflate_results(L, n, raw, ooffs, status, phase, msg, olen, cons, chk):
    return [(status[i], phase[i], L.zs_inflate_message(msg[i]).decode(), raw[ooffs[i]: ooffs[i] + olen[i]], cons[i],
             chk[i]) for i in range(n)]


def _dict_layout(zdict, n):
    """(blob, offsets, lengths) of the inputs' preset dictionaries: one bytes-like for
    all of them, or a sequence with one per input (None / empty = none); equal
    objects are stored once."""
    if isinstance(zdict, (bytes, bytearray, memoryview)):
        zdict = [zdict] * n
    if len(zdict) != n:
        raise ValueError("zdict: %d dictionaries for %d inputs" % (len(zdict), n))
    parts, at, offs, lens, o = [], {}, [], [], 0
    for d in zdict:
        d = b"" if d is None else bytes(d)
        if d and d not in at:
            at[d] = o
            parts.append(d)
            o += len(d)
        offs.append(at[d] if d else 0)
        lens.append(len(d))
    return [b"".join(parts), _arr(ctypes.c_uint64, offs), _arr(ctypes.c_uint32, lens)]


def _layout_shared(inputs):
    """_layout with inputs that are the same object laid out once (many ranges over one file)"""
    seen, parts, offs, lens, o = {}, [], [], [], 0
    for b in inputs:
        if id(b) not in seen:
            seen[id(b)] = o
            parts.append(b)
            o += len(b)
        offs.append(seen[id(b)])
        lens.append(len(b))
    return b"".join(parts), offs, lens


def _inflate_host(L, fn, handle, inputs, fmt, out_caps, check, zdict=(), ranges=None):
    """ranges: decompress_ranges' arrays for a _bgzf_range entry (fn), which takes them behind in_len."""
    n = len(inputs)
    if n == 0:
        return []
    blob, offs, lens = _layout(inputs) if ranges is None else _layout_shared(inputs)
    # the caller's capacities exactly (Z_BUF_ERROR past them); the host entries decode into their own
    # word-aligned staging and copy out only the produced bytes, so these regions need no alignment
    caps = [min(0xffffffff, int(c)) for c in out_caps]
    ooffs, oo = [], 0
    for c in caps:
        ooffs.append(oo)
        oo += c
    out = ctypes.create_string_buffer(max(1, oo))
    res = [(ctypes.c_int32 * n)() for _ in range(3)] + [(ctypes.c_uint32 * n)() for _ in range(3)]
    r = fn(handle, decompress_wbits(fmt), n, blob, _arr(ctypes.c_uint64, offs), _arr(ctypes.c_uint32, lens),
           *(ranges or ()), out, _arr(ctypes.c_uint64, ooffs), _arr(ctypes.c_uint32, caps), *res, *zdict)
    check(r, "inflate batch")
    return _inflate_results(L, n, out.raw, ooffs, *res)


def _inflate_host_auto(L, fn, handle, inputs, fmt, check, zdict=()):
    n = len(inputs)
    if n == 0:
        return []
    blob, offs, lens = _layout(inputs)
    res = [(ctypes.c_int32 * n)() for _ in range(3)] + [(ctypes.c_uint32 * n)() for _ in range(3)]
    ooffs = (ctypes.c_uint64 * n)()
    outp = _P()
    r = fn(handle, decompress_wbits(fmt), n, blob, _arr(ctypes.c_uint64, offs), _arr(ctypes.c_uint32, lens),
           ctypes.byref(outp), ooffs, *res, *zdict)
    check(r, "inflate batch")
    try:
        olen = res[3]
        total = max((ooffs[i] + olen[i] for i in range(n)), default=0)
        raw = ctypes.string_at(outp, total) if total else b""
    finally:
        L.zs_free(outp)
    return _inflate_results(L, n, raw, list(ooffs), *res)


def _ok_or_raise_c(results):
    out = []
    for st, b in results:
        if st != Z_STREAM_END:
            raise ZsError(stream_error_text(st, PHASE_FINISH), st, PHASE_FINISH)
        out.append(b)
    return out


def _ok_or_raise_d(results):
    out = []
    for st, ph, msg, b, _ in results:
        if st != Z_STREAM_END:
            raise ZsError(stream_error_text(st, ph), st, ph, msg)
        out.append(b)
    return out


class Pool:
    """A multi-GPU batch engine (zs_pool, SURVEY.md 8(b) device mask / 8(e)): one
    context per device; each batch is split into contiguous stream ranges, one
    per device, run in parallel -- results identical to one device's."""

    def __init__(self, devices: Optional[Sequence[int]] = None, repeat: bool = False):
        """devices: device indices (None / empty: every visible device).  repeat=True
        takes the list as given, in shard order, a device possibly more than once
        (zs_pool_create_list: the sharding rehearsed on one GPU)."""
        L = lib()
        p = _P()
        if repeat:
            ds = [int(d) for d in devices or []]
            r = L.zs_pool_create_list((ctypes.c_int * max(1, len(ds)))(*ds), len(ds), ctypes.byref(p))
        else:
            mask = 0
            for d in devices or []:
                if not 0 <= int(d) < 64:  # the C mask is 64 bits (ctypes would truncate it to "every device")
                    raise ValueError("device index %r outside 0..63" % (d,))
                mask |= 1 << int(d)
            r = L.zs_pool_create(mask, ctypes.byref(p))
        if r != 0:
            err = L.zs_last_error().decode()
            if r == Z_STREAM_ERROR and ("device mask" in err or "device list" in err or "invalid arg" in err):
                raise ValueError(err)
            raise ZsUnavailable("zs_pool_create failed: %s" % err)
        self._L, self._pool = L, p
        self.devices = [L.zs_pool_device(p, k) for k in range(L.zs_pool_size(p))]

    def close(self):
        if getattr(self, "_pool", None):
            self._L.zs_pool_destroy(self._pool)
            self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, r: int, what: str):
        Engine._check(self, r, what)

    def compress_batch_detailed(self, inputs, fmt="deflate-raw", level=-1, zdict=None, strategy=0, window_bits=None,
                                mem_level=8, flush_at=None, flush_every=None, bgzf=None, primed=False):
        primed = compress_primed(primed, flush_at, flush_every, bgzf)
        block = compress_bgzf(bgzf, fmt, zdict, strategy, window_bits, mem_level, flush_at, flush_every)
        if block is not None:
            return _deflate_host_bgzf(self._L, self._L.zs_pool_deflate_batch_bgzf, self._pool, inputs, level,
                                      self._check, block)
        compress_strategy(strategy, zdict)
        code = compress_params(fmt, window_bits, mem_level, zdict, strategy)
        per = compress_flush([len(b) for b in inputs], flush_at, flush_every, zdict, strategy, window_bits, mem_level)
        if per is not None:
            fn = self._L.zs_pool_deflate_batch_primed if primed else self._L.zs_pool_deflate_batch_flush
            return _deflate_host(self._L, fn, self._pool, inputs, fmt, level, self._check, flush=per, primed=primed)
        if not _params_default(window_bits, mem_level):
            return _deflate_host(self._L, self._L.zs_pool_deflate_batch_params, self._pool, inputs, fmt, level,
                                 self._check, params=(code, mem_level))
        if compress_strategy(strategy, zdict):
            return _deflate_host(self._L, self._L.zs_pool_deflate_batch_strategy, self._pool, inputs, fmt, level,
                                 self._check, strategy=strategy)
        if zdict is not None:
            return _deflate_host(self._L, self._L.zs_pool_deflate_batch_dict, self._pool, inputs, fmt, level,
                                 self._check, _dict_layout(zdict, len(inputs)))
        return _deflate_host(self._L, self._L.zs_pool_deflate_batch, self._pool, inputs, fmt, level, self._check)

    def compress_batch_raw(self, inputs, fmt="deflate-raw", level=-1, zdict=None, strategy=0, window_bits=None,
                           mem_level=8, flush_at=None, flush_every=None, bgzf=None, primed=False):
        return [(st, b) for st, b, _ in self.compress_batch_detailed(inputs, fmt, level, zdict, strategy, window_bits,
                                                                     mem_level, flush_at, flush_every, bgzf, primed)]

    def compress_batch(self, inputs, fmt="deflate-raw", level=-1, zdict=None, strategy=0, window_bits=None,
                       mem_level=8, flush_at=None, flush_every=None, bgzf=None, primed=False):
        return _ok_or_raise_c(self.compress_batch_raw(inputs, fmt, level, zdict, strategy, window_bits, mem_level,
                                                      flush_at, flush_every, bgzf, primed))

    def decompress_batch_detailed(self, inputs, fmt="deflate-raw", out_caps=None, zdict=None, restart=None, members=False,
                                  ranges=None):
        L = self._L
        rng = decompress_ranges(ranges, members, len(inputs))
        mode = decompress_members(members, fmt, out_caps, zdict, restart)  # (zs_last_members is not offered on the pool)
        if rng is not None:
            caps = bgzf_range_out_caps(inputs, ranges) if out_caps is None else out_caps
            return _inflate_host(L, L.zs_pool_inflate_batch_bgzf_range, self._pool, inputs, fmt, caps, self._check, ranges=rng)
        if mode == "bgzf":
            caps = bgzf_out_caps(inputs) if out_caps is None else out_caps
            return _inflate_host(L, L.zs_pool_inflate_batch_bgzf, self._pool, inputs, fmt, caps, self._check)
        if mode:
            return _inflate_host(L, L.zs_pool_inflate_batch_members, self._pool, inputs, fmt, out_caps, self._check)
        if decompress_scan(restart, out_caps, zdict):
            return _inflate_host(L, L.zs_pool_inflate_batch_sync, self._pool, inputs, fmt, out_caps, self._check)
        if restart is not None:  # (zs_last_flush_index is not offered on the pool: an index comes from an Engine)
            rs = decompress_restart(inputs, fmt, restart, out_caps, zdict)
            return _inflate_host(L, L.zs_pool_inflate_batch_restart, self._pool, inputs, fmt, out_caps, self._check, rs)
        if zdict is not None:
            d = _dict_layout(zdict, len(inputs))
            if out_caps is None:
                return _inflate_host_auto(L, L.zs_pool_inflate_batch_dict_auto, self._pool, inputs, fmt, self._check, d)
            return _inflate_host(L, L.zs_pool_inflate_batch_dict, self._pool, inputs, fmt, out_caps, self._check, d)
        if out_caps is None:
            return _inflate_host_auto(L, L.zs_pool_inflate_batch_auto, self._pool, inputs, fmt, self._check)
        return _inflate_host(L, L.zs_pool_inflate_batch, self._pool, inputs, fmt, out_caps, self._check)

    def decompress_batch_raw(self, inputs, fmt="deflate-raw", out_caps=None, zdict=None, restart=None, members=False,
                             ranges=None):
        return [r[:5] for r in self.decompress_batch_detailed(inputs, fmt, out_caps, zdict, restart, members, ranges)]

    def decompress_batch(self, inputs, fmt="deflate-raw", out_caps=None, zdict=None, restart=None, members=False,
                         ranges=None):
        return _ok_or_raise_d(self.decompress_batch_raw(inputs, fmt, out_caps, zdict, restart, members, ranges))


_default: Optional[Engine] = None


def default_engine() -> Engine:
    global _default
    if _default is None:
        _default = Engine(0)
    return _default


def compress_batch(inputs: Sequence[bytes], fmt: str = "deflate-raw", level: int = -1) -> List[bytes]:
    return default_engine().compress_batch(inputs, fmt, level)


def decompress_batch(inputs: Sequence[bytes], fmt: str = "deflate-raw") -> List[bytes]:
    return default_engine().decompress_batch(inputs, fmt)


class _OneShotStream:
    """write()/close()/read() over a single-stream GPU batch (streams.ts semantics:
    the whole input is collected, then processed as ONE write() + close())."""

    def __init__(self):
        self._chunks: List[bytes] = []
        self._out: Optional[bytes] = None

    def write(self, chunk: bytes):
        if self._out is not None:
            raise ZsError("stream closed")
        self._chunks.append(bytes(chunk))

    def read(self) -> bytes:
        if self._out is None:
            raise ZsError("stream not closed")
        return self._out


class CompressionStream(_OneShotStream):
    """streams.ts:242-251 (format 'deflate' | 'gzip' | 'deflate-raw', {level})."""

    def __init__(self, fmt: str = "deflate", level: Optional[int] = None):
        super().__init__()
        self.format, self.level = fmt, compress_level(level)

    def close(self) -> bytes:
        self._out = default_engine().compress_batch([b"".join(self._chunks)], self.format, self.level)[0]
        return self._out


class DecompressionStream(_OneShotStream):
    """streams.ts:253-262 (format 'deflate' | 'gzip' | 'deflate-raw' | 'deflate64-raw')."""

    def __init__(self, fmt: str = "deflate"):
        super().__init__()
        self.format = fmt

    def close(self) -> bytes:
        self._out = default_engine().decompress_batch([b"".join(self._chunks)], self.format)[0]
        return self._out


def corpus(kind: str, first_index: int, n_streams: int, length: int, threads: int = 8) -> bytearray:
    """Synthetic T ('text') / M ('mixed') / 'rand' corpora."""
    k = {"text": 0, "mixed": 1, "rand": 2}[kind]
    buf = bytearray(n_streams * length)
    cbuf = (ctypes.c_char * len(buf)).from_buffer(buf)
    lib().zs_corpus(k, first_index, n_streams, length, ctypes.cast(cbuf, _P), threads)
    return buf
