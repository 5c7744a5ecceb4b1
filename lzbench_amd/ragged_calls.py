"""The ragged device calls of include/lzbench_hip.h 3b .. 3i as a table: one RaggedCall per async entry point.

The calls share one argument list per direction and differ in a head (the arguments before the chunk arrays), in
whether the batch's promised total follows max_chunk_bytes, and in their sizing calls.  The ctypes signatures of
lzbench_amd.SIGNATURES, RaggedCodec's dispatch and the check-order test (tests/test_ragged_calls_abi.py) are all read
from RAGGED_CALLS, the calls of 3b .. 3g.  A later call is one more row in MORE_CALLS: signatures(), COMPRESS and
DECOMPRESS cover both tuples, while the check-order test and tests/ragged_fake.py stay with the rows they were written
for (a later call brings its own check-order test).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

_P, _SZ = C.c_void_p, C.c_size_t
# every argument of a ragged call or of a sizing call, by name (the head kinds: codec, level, dict, dict_bytes)
ARG_TYPES = dict(
    codec=C.c_int, level=C.c_int, dict=_P, dict_bytes=_SZ, total=_SZ, nchunks=_SZ, max_chunk_bytes=_SZ,
    in_ptrs=_P, in_bytes=_P, out_ptrs=_P, out_bytes=_P, packed=_P, packed_cap=_SZ, packed_readable=_SZ, csizes=_P,
    offsets=_P, status=_P, temp=_P, temp_bytes=_SZ, stream=_P)
# after the head (total: only where the call takes the promise)
_COMPRESS_ARGS = ("in_ptrs", "in_bytes", "nchunks", "max_chunk_bytes", "total", "packed", "packed_cap", "csizes",
                  "offsets", "temp", "temp_bytes", "stream")
_DECOMPRESS_ARGS = ("packed", "packed_readable", "csizes", "offsets", "out_ptrs", "out_bytes", "nchunks",
                    "max_chunk_bytes", "total", "status", "temp", "temp_bytes", "stream")


class _Call:
    """A C function whose arguments are passed by name: f(lib, **values) takes the ones in f.names."""

    def signature(self):
        return self.restype, [ARG_TYPES[n] for n in self.names]

    def __call__(self, lib, **values):
        return getattr(lib, self.symbol)(*(values[n] for n in self.names))


@dataclass(frozen=True)
class Sizing(_Call):
    """A *_temp_bytes function: head, then max_chunk_bytes and nchunks; 0 where the call refuses the arguments."""
    symbol: str
    head: Tuple[str, ...] = ()     # of codec, level, dict_bytes, total
    restype = _SZ

    @property
    def names(self):
        return self.head + ("max_chunk_bytes", "nchunks")


@dataclass(frozen=True)
class RaggedCall(_Call):
    symbol: str
    compress: bool                   # (else decompress)
    family: str                      # RaggedCodec's variant: lz, lz4_dict, zstd, zstd_dfast, zstd_dict, zstd_dfast_dict, lz4f
    head: Tuple[str, ...]            # of codec, level, dict, dict_bytes
    sizing: Sizing                   # the temp below which the call answers LZH_ESPACE
    promise: bool = False            # the compact layouts: the batch's promised total follows max_chunk_bytes
    nullable: Tuple[str, ...] = ()   # pointers that may be null (decode: offsets are then scanned into temp)
    # decode: the larger temp in which the call runs the split decoder; at 0 (no split decoder for chunks of this size)
    # and below its answer the call falls back to the one-wave kernel and the temp of `sizing`
    roomy: Optional[Sizing] = None
    # launch blocks per chunk (api.cpp: nchunks * grid_factor > 0x7fffffff is refused): the calls of 3b pass the 64 KiB
    # fragments of max_chunk_bytes, the snappy parse kernel's grid, for either codec; every other call 1
    grid_frags: bool = False
    restype = C.c_int

    @property
    def names(self):
        tail = _COMPRESS_ARGS if self.compress else _DECOMPRESS_ARGS
        return self.head + tuple(n for n in tail if n != "total" or self.promise)

    @property
    def required_pointers(self):
        return tuple(n for n in self.names if ARG_TYPES[n] is _P and n != "stream" and n not in self.nullable)

    def grid_factor(self, max_chunk_bytes: int) -> int:
        return max(1, (max_chunk_bytes + 65535) >> 16) if self.grid_frags else 1

    def temp_bytes(self, lib, roomy: bool = False, **values) -> int:
        """The temp to allocate (0: arguments the call refuses); roomy: `roomy`'s answer where there is one."""
        return (roomy and self.roomy is not None and self.roomy(lib, **values)) or self.sizing(lib, **values)


def _c(symbol, family, head, sizing, **kw):
    return RaggedCall(symbol, True, family, head, sizing, **kw)


def _d(symbol, family, head, sizing, **kw):
    return RaggedCall(symbol, False, family, head, sizing, nullable=("offsets",), **kw)


_ZSTD_SMALL = Sizing("lzh_zstd_ragged_decompress_temp_bytes")
_DICT = ("dict", "dict_bytes")
RAGGED_CALLS = (
    # 3b: LZ4 / snappy
    _c("lzh_compress_ragged_async", "lz", ("codec", "level"), Sizing("lzh_ragged_compress_temp_bytes", ("codec",)),
       grid_frags=True),
    _c("lzh_compress_ragged_compact_async", "lz", ("codec", "level"),
       Sizing("lzh_ragged_compact_compress_temp_bytes", ("codec", "total")), promise=True, grid_frags=True),
    _d("lzh_decompress_ragged_async", "lz", ("codec",), Sizing("lzh_ragged_decompress_temp_bytes", ("codec",))),
    # 3c: zstd, the fast-strategy levels
    _c("lzh_zstd_compress_ragged_async", "zstd", ("level",), Sizing("lzh_zstd_ragged_compress_temp_bytes", ("level",))),
    _c("lzh_zstd_compress_ragged_compact_async", "zstd", ("level",),
       Sizing("lzh_zstd_ragged_compact_compress_temp_bytes", ("level", "total")), promise=True),
    _d("lzh_zstd_decompress_ragged_async", "zstd", (), _ZSTD_SMALL,
       roomy=Sizing("lzh_zstd_ragged_decompress_split_temp_bytes")),
    # 3d: LZ4 with a shared dictionary
    _c("lzh_lz4_compress_ragged_dict_async", "lz4_dict", ("level",) + _DICT,
       Sizing("lzh_lz4_dict_compress_temp_bytes", ("dict_bytes",))),
    _d("lzh_lz4_decompress_ragged_dict_async", "lz4_dict", _DICT,
       Sizing("lzh_lz4_dict_decompress_temp_bytes", ("dict_bytes",))),
    # 3e: zstd level 3 (the frames decode with 3c's calls)
    _c("lzh_zstd_dfast_compress_ragged_async", "zstd_dfast", ("level",),
       Sizing("lzh_zstd_dfast_ragged_compress_temp_bytes", ("level",))),
    _c("lzh_zstd_dfast_compress_ragged_compact_async", "zstd_dfast", ("level",),
       Sizing("lzh_zstd_dfast_ragged_compact_compress_temp_bytes", ("level", "total")), promise=True),
    # 3f: zstd with a shared dictionary
    _c("lzh_zstd_compress_ragged_dict_async", "zstd_dict", ("level",) + _DICT,
       Sizing("lzh_zstd_dict_compress_temp_bytes", ("level", "dict_bytes"))),
    _d("lzh_zstd_decompress_ragged_dict_async", "zstd_dict", _DICT,
       Sizing("lzh_zstd_dict_decompress_temp_bytes", ("dict_bytes",))),
    # 3g: 3c's decoder, the split decoder's temp sized from the promised total
    _d("lzh_zstd_decompress_ragged_split_compact_async", "zstd", (), _ZSTD_SMALL, promise=True,
       roomy=Sizing("lzh_zstd_ragged_decompress_split_compact_temp_bytes", ("total",))),
)
MORE_CALLS = (
    # 3h: zstd level 3 with a shared dictionary (the frames decode with 3f's call)
    _c("lzh_zstd_dfast_compress_ragged_dict_async", "zstd_dfast_dict", ("level",) + _DICT,
       Sizing("lzh_zstd_dfast_dict_compress_temp_bytes", ("level", "dict_bytes"))),
    # 3i: LZ4 frames, a frame per chunk (level = LZH_LZ4F_PARAMS; independent blocks)
    _c("lzh_lz4f_compress_ragged_async", "lz4f", ("level",), Sizing("lzh_lz4f_ragged_compress_temp_bytes", ("level",))),
    _d("lzh_lz4f_decompress_ragged_async", "lz4f", (), Sizing("lzh_lz4f_ragged_decompress_temp_bytes")),
)
ALL_CALLS = RAGGED_CALLS + MORE_CALLS
# RaggedCodec's lookup: (family, compact layout) -> the call
COMPRESS = {(r.family, r.promise): r for r in ALL_CALLS if r.compress}
DECOMPRESS = {(r.family, r.promise): r for r in ALL_CALLS if not r.compress}


def signatures() -> dict:
    """The SIGNATURES entries of the calls and of their sizing functions."""
    every = [f for r in ALL_CALLS for f in (r, r.sizing, r.roomy) if f is not None]
    return {f.symbol: f.signature() for f in every}
