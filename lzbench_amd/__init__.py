"""lzbench_amd -- host-side mirror of lzbench's compressor_desc_t table and chunk loop for the
MI355X (gfx950) LZ4 / snappy codecs of liblzbench_hip.so.

Reference interface mirrored here:
  * compressor_desc_t rows ........ /root/reference/_lzbench/lzbench.h:113-129, :140-219
  * lzbench_compress / _decompress  /root/reference/_lzbench/lzbench.cpp:266-298 / :301-329
    (raw-store rule clen <= 0 || clen == part, contiguous packing, compr_sizes[])
  * GET_COMPRESS_BOUND ............ /root/reference/_lzbench/lzbench.h:17

Everything here is a thin ctypes layer over the C-ABI in include/lzbench_hip.h; the codec
work runs in the HIP kernels of lzbench_amd/csrc.  There is no CPU fallback: if the shared
library is missing the import of any codec entry point raises ExtensionMissing.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import ragged_calls

__all__ = [
    "ExtensionMissing", "lib", "CODECS", "COMP_DESC", "CompressorDesc", "find_compressor",
    "compress_chunks", "decompress_chunks", "chunk_sizes_for", "datagen", "DeviceCodec", "RaggedCodec",
    "LZH_CODEC_LZ4", "LZH_CODEC_SNAPPY", "LZH_CODEC_MEMCPY", "LZH_CODEC_ZSTD", "LZH_CODEC_LZ4F", "LZH_CODEC_NVLZ4",
    "LZH_CODEC_ZSTD_DFAST",
    "LZ4F_BLOCK_CHECKSUM", "LZ4F_CONTENT_CHECKSUM", "LZ4F_CONTENT_SIZE", "LZ4F_LINKED", "PAD_SIZE",
    "get_compress_bound",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
# LZH_LIB: an alternative in-tree build of the same library (kernel experiments; tools/exp_build.sh)
LIB_PATH = os.environ.get("LZH_LIB") or os.path.join(_HERE, "liblzbench_hip.so")
DATAGEN_PATH = os.path.join(_HERE, "libdatagen.so")

LZH_CODEC_LZ4, LZH_CODEC_SNAPPY, LZH_CODEC_MEMCPY, LZH_CODEC_ZSTD, LZH_CODEC_LZ4F, LZH_CODEC_NVLZ4 = 0, 1, 2, 3, 4, 5
LZH_CODEC_ZSTD_DFAST = 6      # zstd level 3 (the double-fast strategy): LZH_CODEC_ZSTD's frames, a codec of its own
CODECS = {"lz4": LZH_CODEC_LZ4, "lz4fast": LZH_CODEC_LZ4, "snappy": LZH_CODEC_SNAPPY, "memcpy": LZH_CODEC_MEMCPY,
          "zstd": LZH_CODEC_ZSTD, "zstd_fast": LZH_CODEC_ZSTD, "lz4frame": LZH_CODEC_LZ4F,
          "nvcomp_lz4": LZH_CODEC_NVLZ4, "zstd_dfast": LZH_CODEC_ZSTD_DFAST}
# LZ4 frame parameters (include/lzbench_hip.h LZH_LZ4F_*): level = bsid | flags | acceleration << 8
LZ4F_BLOCK_CHECKSUM, LZ4F_CONTENT_CHECKSUM, LZ4F_CONTENT_SIZE, LZ4F_LINKED = 0x10, 0x20, 0x40, 0x80
# codecs whose level is passed through as is (the others: 1 for lz4 = LZ4_compress_default, 0)
_LEVELED = ("lz4fast", "zstd", "zstd_fast", "zstd_dfast", "lz4frame", "nvcomp_lz4")
PAD_SIZE = 16 * 1024          # lzbench.h:14


def get_compress_bound(n: int) -> int:
    """GET_COMPRESS_BOUND (lzbench.h:17)."""
    return n + n // 6 + PAD_SIZE


class ExtensionMissing(RuntimeError):
    """liblzbench_hip.so is not built (run __graft_entry__.build())."""


_P = C.c_void_p
_SZ = C.c_size_t
_I64 = C.c_int64
_lib = None
_dg = None

# exported symbols and their signatures (restype, argtypes) -- kept in sync with
# include/lzbench_hip.h; tests/test_abi.py checks every header declaration is here and loads
_COMPRESS_FUNC = (_I64, [_P, _SZ, _P, _SZ, _SZ, _SZ, _P])
SIGNATURES = {
    "lzbench_hip_lz4_init": (_P, [_SZ, _SZ, _SZ]),
    "lzbench_hip_snappy_init": (_P, [_SZ, _SZ, _SZ]),
    "lzbench_hip_memcpy_init": (_P, [_SZ, _SZ, _SZ]),
    "lzbench_hip_zstd_init": (_P, [_SZ, _SZ, _SZ]),
    "lzbench_hip_zstd_dfast_init": (_P, [_SZ, _SZ, _SZ]),
    "lzbench_hip_zstd_dfast_compress": _COMPRESS_FUNC,
    "lzbench_hip_lz4frame_init": (_P, [_SZ, _SZ, _SZ]),
    "lzbench_hip_nvcomp_lz4_init": (_P, [_SZ, _SZ, _SZ]),
    "lzbench_hip_lz4frame_compress": _COMPRESS_FUNC,
    "lzbench_hip_lz4frame_decompress": _COMPRESS_FUNC,
    "lzbench_hip_nvcomp_lz4_compress": _COMPRESS_FUNC,
    "lzbench_hip_nvcomp_lz4_decompress": _COMPRESS_FUNC,
    "lzbench_hip_zstd_compress": _COMPRESS_FUNC,
    "lzbench_hip_zstd_decompress": _COMPRESS_FUNC,
    "lzbench_hip_deinit": (None, [_P]),
    "lzbench_hip_lz4_compress": _COMPRESS_FUNC,
    "lzbench_hip_lz4fast_compress": _COMPRESS_FUNC,
    "lzbench_hip_lz4_decompress": _COMPRESS_FUNC,
    "lzbench_hip_snappy_compress": _COMPRESS_FUNC,
    "lzbench_hip_snappy_decompress": _COMPRESS_FUNC,
    "lzbench_hip_memcpy": _COMPRESS_FUNC,
    "lzbench_hip_compress_batch": (_I64, [_P, _P, C.c_int, _P, _SZ, _P, _SZ, _SZ, _P]),
    "lzbench_hip_decompress_batch": (_I64, [_P, _P, _P, C.c_int, _P, _SZ, _SZ, _SZ, _P]),
    "lzh_stage_stride": (_SZ, [C.c_int, _SZ]),
    "lzh_max_packed_bytes": (_SZ, [C.c_int, _SZ, _SZ]),
    "lzh_compress_temp_bytes": (_SZ, [C.c_int, _SZ, _SZ]),
    "lzh_decompress_temp_bytes": (_SZ, [C.c_int, _SZ, _SZ]),
    "lzh_num_chunks": (_SZ, [_SZ, _SZ]),
    "lzh_level_supported": (C.c_int, [C.c_int, C.c_int, _SZ]),
    "lzh_debug_plan": (C.c_int, [_SZ, _SZ, _SZ, C.c_int, _P, C.c_int]),
    "lzh_debug_gather_order": (C.c_int, [_SZ, _P, _P, _P]),
    "lzh_compress_async": (C.c_int, [C.c_int, C.c_int, _P, _SZ, _SZ, _SZ, _P, _SZ, _P, _P, _P, _SZ, _P]),
    "lzh_decompress_async": (C.c_int, [C.c_int, _P, _SZ, _P, _P, _SZ, _SZ, _P, _P, _P, _SZ, _P]),
    "lzh_ragged_max_packed_bytes": (_SZ, [C.c_int, _SZ, _SZ]),
    "lzh_zstd_ragged_max_packed_bytes": (_SZ, [_SZ, _SZ]),
    "lzh_lz4f_ragged_max_packed_bytes": (_SZ, [_SZ, _SZ]),
    "lzh_debug_zstd_ragged_split_layout": (C.c_int, [_SZ, _SZ, _P]),
    "lzh_debug_zstd_ragged_split_compact_slots": (C.c_int, [_P, _SZ, _SZ, _SZ, _P, _P, _P]),
    "lzh_debug_zstd_ragged_split_compact_layout": (C.c_int, [_SZ, _SZ, _SZ, _P]),
    "lzh_debug_zstd_ragged_compact_slots": (C.c_int, [C.c_int, _P, _SZ, _SZ, _SZ, _P, _P, _P]),
    "lzh_debug_zstd_ragged_compact_regions": (C.c_int, [C.c_int, _SZ, _SZ, _SZ, _P]),
    "lzh_debug_zstd_dfast_ragged_compact_slots": (C.c_int, [C.c_int, _P, _SZ, _SZ, _SZ, _P, _P, _P]),
    "lzh_debug_zstd_dfast_ragged_compact_regions": (C.c_int, [C.c_int, _SZ, _SZ, _SZ, _P]),
    "lzh_debug_ragged_compact_slots": (C.c_int, [C.c_int, _P, _SZ, _SZ, _SZ, _P, _P, _P]),
    "lzh_debug_ragged_compact_regions": (C.c_int, [C.c_int, _SZ, _SZ, _SZ, _P]),
    "lzh_debug_zstd_dict_params": (C.c_int, [C.c_int, _SZ, _SZ, _P]),
    "lzh_debug_zstd_dict_parse": (C.c_long, [C.c_int, _P, _SZ, _P, _SZ, _P, _SZ]),
    "lzh_compress_kernel_only": (C.c_int, [C.c_int, C.c_int, _P, _SZ, _SZ, _SZ, _P, _P, _P]),
    "lzh_compress_kernel_stage": (C.c_int, [C.c_int, C.c_int, C.c_int, _P, _SZ, _SZ, _SZ, _P, _P, _P]),
    "lzh_compress_finish_async": (C.c_int, [C.c_int, _P, _SZ, _SZ, _SZ, _P, _P, _P, _SZ, _P, _P]),
    "lzh_datagen": (_SZ, [C.c_int, C.c_uint64, _P, _SZ]),
    "lzh_version": (C.c_char_p, []),
    "lzh_debug_zstd_dfast_dict_params": (C.c_int, [C.c_int, _SZ, _SZ, _P]),
    "lzh_debug_zstd_dfast_dict_parse": (C.c_long, [C.c_int, _P, _SZ, _P, _SZ, _P, _SZ, _P]),
    # the ragged async calls of 3b .. 3i and their *_temp_bytes functions: generated from the table
    **ragged_calls.signatures(),
}


def lib():
    """The loaded C-ABI library (raises ExtensionMissing if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ExtensionMissing(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            # (an older experiment build named by LZH_LIB may lack the newest debug entry points)
            if os.environ.get("LZH_LIB") and name.startswith("lzh_debug") and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def datagen(kind: str | int, n: int, seed: int = 12345, offset: int = 0) -> np.ndarray:
    """Synthetic corpus: random / text / json / mixed / binary.  offset (a multiple
    of 16 MiB): bytes [offset, offset + n) of the same corpus -- a rank's share of a multi-GiB input
    (the corpus is generated in independent 16 MiB segments, so a share needs no prefix)."""
    global _dg
    kinds = {"random": 0, "text": 1, "json": 2, "mixed": 3, "binary": 4}
    k = kinds[kind] if isinstance(kind, str) else int(kind)
    if _dg is None:
        if not os.path.exists(DATAGEN_PATH):
            raise ExtensionMissing(f"{DATAGEN_PATH} not found")
        _dg = C.CDLL(DATAGEN_PATH)
        _dg.lzb_datagen.restype = _SZ
        _dg.lzb_datagen.argtypes = [C.c_int, C.c_uint64, _P, _SZ]
        _dg.lzb_datagen_at.restype = _SZ
        _dg.lzb_datagen_at.argtypes = [C.c_int, C.c_uint64, _P, _SZ, _SZ]
    if offset % (16 << 20):
        raise ValueError("datagen offset must be a multiple of 16 MiB")
    buf = np.empty(max(n, 1), dtype=np.uint8)
    if _dg.lzb_datagen_at(k, C.c_uint64(seed), buf.ctypes.data, offset, n) != n:
        raise ValueError(f"bad corpus kind {kind}")
    return buf[:n]


@dataclass(frozen=True)
class CompressorDesc:
    """One row of lzbench's comp_desc[] (lzbench.h:117-129); function fields name C symbols."""
    name: str
    version: str
    first_level: int
    last_level: int
    additional_param: int
    max_block_size: int
    compress: Optional[str]
    decompress: Optional[str]
    init: Optional[str]
    deinit: Optional[str]
    compress_batch: Optional[str] = None
    decompress_batch: Optional[str] = None


# index 0 stays memcpy (lzbench.cpp:609, :695); the GPU rows replace cudaMemcpy / nvcomp_lz4
# (lzbench.h:217-218) and add bit-exact lz4 / lz4fast / snappy rows.
COMP_DESC = (
    CompressorDesc("memcpy", "", 0, 0, 0, 0, None, None, None, None),
    CompressorDesc("hipMemcpy", "", 0, 0, 1, 0, "lzbench_hip_memcpy", "lzbench_hip_memcpy",
                   "lzbench_hip_memcpy_init", "lzbench_hip_deinit",
                   "lzbench_hip_compress_batch", "lzbench_hip_decompress_batch"),
    CompressorDesc("hip_lz4", "1.9.3", 0, 0, 1, 0, "lzbench_hip_lz4_compress", "lzbench_hip_lz4_decompress",
                   "lzbench_hip_lz4_init", "lzbench_hip_deinit",
                   "lzbench_hip_compress_batch", "lzbench_hip_decompress_batch"),
    CompressorDesc("hip_lz4fast", "1.9.3", 1, 99, 1, 0, "lzbench_hip_lz4fast_compress", "lzbench_hip_lz4_decompress",
                   "lzbench_hip_lz4_init", "lzbench_hip_deinit",
                   "lzbench_hip_compress_batch", "lzbench_hip_decompress_batch"),
    CompressorDesc("hip_snappy", "2020-07-11", 0, 0, 1, 0, "lzbench_hip_snappy_compress",
                   "lzbench_hip_snappy_decompress", "lzbench_hip_snappy_init", "lzbench_hip_deinit",
                   "lzbench_hip_compress_batch", "lzbench_hip_decompress_batch"),
    # zstd / zstd_fast rows (lzbench.h:209-210) restricted to the fast-strategy levels
    CompressorDesc("hip_zstd", "1.5.2", 1, 2, 1, 0, "lzbench_hip_zstd_compress", "lzbench_hip_zstd_decompress",
                   "lzbench_hip_zstd_init", "lzbench_hip_deinit",
                   "lzbench_hip_compress_batch", "lzbench_hip_decompress_batch"),
    CompressorDesc("hip_zstd_fast", "1.5.2", -5, -1, 1, 0, "lzbench_hip_zstd_compress", "lzbench_hip_zstd_decompress",
                   "lzbench_hip_zstd_init", "lzbench_hip_deinit",
                   "lzbench_hip_compress_batch", "lzbench_hip_decompress_batch"),
    # zstd's default level: the double-fast strategy, a codec of its own (LZH_CODEC_ZSTD_DFAST); same frames
    CompressorDesc("hip_zstd_dfast", "1.5.2", 3, 3, 1, 0, "lzbench_hip_zstd_dfast_compress",
                   "lzbench_hip_zstd_decompress", "lzbench_hip_zstd_dfast_init", "lzbench_hip_deinit",
                   "lzbench_hip_compress_batch", "lzbench_hip_decompress_batch"),
    # framed formats: an LZ4 frame per chunk (level = LZH_LZ4F_PARAMS), the nvcomp_lz4 row's container
    # (lzbench.h:218, levels 0..5 = chunks of 32 KiB << level)
    CompressorDesc("hip_lz4frame", "1.9.3", 4, 7, 1, 0, "lzbench_hip_lz4frame_compress",
                   "lzbench_hip_lz4frame_decompress", "lzbench_hip_lz4frame_init", "lzbench_hip_deinit",
                   "lzbench_hip_compress_batch", "lzbench_hip_decompress_batch"),
    CompressorDesc("hip_nvcomp_lz4", "1.2.2", 0, 5, 1, 0, "lzbench_hip_nvcomp_lz4_compress",
                   "lzbench_hip_nvcomp_lz4_decompress", "lzbench_hip_nvcomp_lz4_init", "lzbench_hip_deinit",
                   "lzbench_hip_compress_batch", "lzbench_hip_decompress_batch"),
)


def find_compressor(name: str) -> CompressorDesc:
    """Name lookup as in lzbench_test_with_params (lzbench.cpp:492-530); plain codec names
    (lz4, lz4fast, snappy) resolve to their GPU rows."""
    for d in COMP_DESC:
        if d.name == name or d.name == "hip_" + name:
            return d
    raise KeyError(f"{name} NOT FOUND")


def chunk_sizes_for(n: int, chunk_size: int) -> np.ndarray:
    """lzbench_test's chunk list for one file (lzbench.cpp:366-373)."""
    k = (n + chunk_size - 1) // chunk_size
    cs = np.full(k, chunk_size, dtype=np.uint64)
    if k and n % chunk_size:
        cs[-1] = n % chunk_size
    return cs


def _as_u8(a) -> np.ndarray:
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(a), dtype=np.uint8)
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


class _Row:
    """An init'ed GPU row (workmem owner)."""

    def __init__(self, codec: str, chunk_size: int, level: int = 0, ngpus: int = 1):
        L = lib()
        base = {"memcpy": "memcpy", "snappy": "snappy", "zstd": "zstd", "zstd_fast": "zstd", "zstd_dfast": "zstd_dfast",
                "lz4frame": "lz4frame",
                "nvcomp_lz4": "nvcomp_lz4"}.get(codec, "lz4")
        self.desc = find_compressor("hipMemcpy" if codec == "memcpy" else codec)
        self.wm = getattr(L, f"lzbench_hip_{base}_init")(chunk_size, level, ngpus)
        if not self.wm:
            raise RuntimeError("lzbench_hip init failed (no HIP device?)")
        self.level = level

    def close(self):
        if self.wm:
            lib().lzbench_hip_deinit(self.wm)
            self.wm = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _row_level(codec: str, level: int) -> int:
    """The level argument lzbench passes for the row: lz4fast acceleration, zstd level (zstd_fast
    rows are negative), 1 for lz4 (LZ4_compress_default), 0 for snappy; size_t on the wire."""
    if codec in _LEVELED:
        return level & 0xFFFFFFFFFFFFFFFF
    return 1 if codec == "lz4" else 0


def compress_chunks(data, codec: str = "lz4", chunk_size: int = 65536, level: int = 0, ngpus: int = 1,
                    chunk_sizes=None) -> Tuple[np.ndarray, np.ndarray]:
    """lzbench_compress over the chunk list on the GPU(s). Returns (packed bytes, compr_sizes)."""
    src = _as_u8(data)
    cs = np.ascontiguousarray(chunk_sizes if chunk_sizes is not None else chunk_sizes_for(len(src), chunk_size),
                              dtype=np.uint64)
    out = np.zeros(get_compress_bound(len(src)) + 64, dtype=np.uint8)
    compr = np.zeros(len(cs), dtype=np.uint64)
    lvl = _row_level(codec, level)
    with _Row(codec, chunk_size, lvl, ngpus) as row:
        total = lib().lzbench_hip_compress_batch(src.ctypes.data, cs.ctypes.data, len(cs), out.ctypes.data,
                                                 len(out), compr.ctypes.data, lvl, ngpus, row.wm)
    if total <= 0 and len(src) > 0:
        raise RuntimeError(f"compress_batch failed ({total})")
    return out[:total].copy(), compr


def decompress_chunks(packed, compr_sizes, n: int, codec: str = "lz4", chunk_size: int = 65536, ngpus: int = 1,
                      chunk_sizes=None) -> np.ndarray:
    """lzbench_decompress over the chunk list on the GPU(s). Raises on malformed chunks."""
    src = _as_u8(packed)
    cs = np.ascontiguousarray(chunk_sizes if chunk_sizes is not None else chunk_sizes_for(n, chunk_size),
                              dtype=np.uint64)
    comp = np.ascontiguousarray(compr_sizes, dtype=np.uint64)
    out = np.zeros(n + PAD_SIZE, dtype=np.uint8)
    with _Row(codec, chunk_size, 0, ngpus) as row:
        total = lib().lzbench_hip_decompress_batch(src.ctypes.data, comp.ctypes.data, cs.ctypes.data, len(cs),
                                                   out.ctypes.data, len(out), 0, ngpus, row.wm)
    if total != n:
        raise RuntimeError(f"decompress_batch failed ({total})")
    return out[:n]


class DeviceCodec:
    """Device-resident batched codec on HBM tensors (include/lzbench_hip.h layer 3).

    Buffers are torch uint8 CUDA tensors; work is queued on torch's current stream, so
    torch.cuda.Event pairs on that stream time it.
    """

    def __init__(self, codec: str, n: int, chunk_size: int, level: int = 0, device=None):
        import torch
        self.torch = torch
        self.codec = CODECS[codec]
        self.level = level if codec in _LEVELED else (1 if codec == "lz4" else 0)
        self.n, self.chunk_size = n, chunk_size
        L = lib()
        self.k = L.lzh_num_chunks(n, chunk_size)
        dev = device or torch.device("cuda", torch.cuda.current_device())
        u8 = dict(dtype=torch.uint8, device=dev)
        self.max_packed = L.lzh_max_packed_bytes(self.codec, n, chunk_size)
        self.packed = torch.empty(self.max_packed + 64, **u8)
        self.csizes = torch.empty(self.k, dtype=torch.int32, device=dev)
        self.offsets = torch.empty(self.k + 1, dtype=torch.int64, device=dev)
        self.status = torch.empty(self.k, dtype=torch.int32, device=dev)
        self.ctemp = torch.empty(max(L.lzh_compress_temp_bytes(self.codec, n, chunk_size), 256), **u8)
        self.dtemp = torch.empty(max(L.lzh_decompress_temp_bytes(self.codec, n, chunk_size), 256), **u8)
        self.out = torch.empty(n + 64, **u8)

    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def compress(self, d_in, in_readable: Optional[int] = None) -> None:
        rc = lib().lzh_compress_async(self.codec, self.level, d_in.data_ptr(), self.n,
                                      in_readable if in_readable is not None else d_in.numel(), self.chunk_size,
                                      self.packed.data_ptr(), self.packed.numel(), self.csizes.data_ptr(),
                                      self.offsets.data_ptr(), self.ctemp.data_ptr(), self.ctemp.numel(),
                                      self._stream())
        if rc:
            raise RuntimeError(f"lzh_compress_async failed ({rc})")

    def compress_kernel_only(self, d_in) -> None:
        rc = lib().lzh_compress_kernel_only(self.codec, self.level, d_in.data_ptr(), self.n, d_in.numel(),
                                            self.chunk_size, self.ctemp.data_ptr(), self.csizes.data_ptr(),
                                            self._stream())
        if rc:
            raise RuntimeError(f"lzh_compress_kernel_only failed ({rc})")

    def compress_stage(self, d_in, stage_mask: int) -> None:
        """One stage of compress_kernel_only (1 = parse kernel, 2 = LZ4 emission kernel)."""
        rc = lib().lzh_compress_kernel_stage(self.codec, self.level, stage_mask, d_in.data_ptr(), self.n, d_in.numel(),
                                             self.chunk_size, self.ctemp.data_ptr(), self.csizes.data_ptr(),
                                             self._stream())
        if rc:
            raise RuntimeError(f"lzh_compress_kernel_stage failed ({rc})")

    def compress_finish(self, d_in) -> None:
        rc = lib().lzh_compress_finish_async(self.codec, d_in.data_ptr(), self.n, d_in.numel(), self.chunk_size,
                                             self.ctemp.data_ptr(), self.csizes.data_ptr(), self.packed.data_ptr(),
                                             self.packed.numel(), self.offsets.data_ptr(), self._stream())
        if rc:
            raise RuntimeError(f"lzh_compress_finish_async failed ({rc})")

    def decompress(self, packed=None, csizes=None, offsets=None) -> None:
        packed = self.packed if packed is None else packed
        csizes = self.csizes if csizes is None else csizes
        rc = lib().lzh_decompress_async(self.codec, packed.data_ptr(), packed.numel(), csizes.data_ptr(),
                                        offsets.data_ptr() if offsets is not None else None, self.n,
                                        self.chunk_size, self.out.data_ptr(), self.status.data_ptr(),
                                        self.dtemp.data_ptr(), self.dtemp.numel(), self._stream())
        if rc:
            raise RuntimeError(f"lzh_decompress_async failed ({rc})")

    def packed_total(self) -> int:
        return int(self.offsets[self.k].item())


class RaggedCodec:
    """Device-resident codec over ragged batches (include/lzbench_hip.h 3b; zstd: 3c): chunk i of a batch is
    sizes[i] bytes at offsets[i] of a flat uint8 CUDA tensor, any alignment, in any order.

    Buffers are sized once for max_chunks chunks of up to max_chunk_bytes; max_total_bytes bounds a
    batch's total input (default max_chunks * max_chunk_bytes) and sizes `packed`.  The compress temp
    has a staging slot and a sequence-record slot per chunk.  compact=False sizes every slot for
    max_chunk_bytes: a skewed batch pays for its largest chunk max_chunks times.  compact=True sizes
    each slot from its own chunk (lzh_compress_ragged_compact_async): the temp grows with
    max_total_bytes (about 3.2 x) plus some 600 bytes per chunk, the output is the same, and a batch
    must keep its total within max_total_bytes (checked on the host by compress(); compress_arrays()
    leaves a chunk whose slots do not fit uncompressed with csizes[i] = 0).
    zstd / zstd_fast (the fast-strategy levels lzh_level_supported accepts for max_chunk_bytes) go through the
    lzh_zstd_*_ragged calls: one frame per chunk, a staging slot and a scratch area of the zstd kernels per chunk,
    each sized for max_chunk_bytes.  compact_scratch=True (zstd only, else ValueError) sizes both from each chunk's
    own size and the level instead (lzh_zstd_compress_ragged_compact_async): the temp grows with max_total_bytes
    (at most 25 x: a small chunk's hash table is several times the chunk) plus 7.5 KiB per chunk, a large chunk
    pays for one 128 KiB block and not for its size, the temp never passes the other layout's by more than four
    small arrays, the output is the same, and a batch must keep its total within max_total_bytes
    as with compact=True.  compact=True itself raises ValueError for zstd (the LZ4 / snappy calls refuse the
    codec): compact_scratch is the zstd option.
    zstd_dfast (level 3, the double-fast strategy; any other level: ValueError) is zstd in everything above -- the
    frames, compact_scratch (at most 33 x max_total_bytes plus 7.5 KiB per chunk: a frame keeps two tables), the
    refusal of compact=True, the refusal of a dictionary (zstd_dfast has none), the decoder and split_decode below -- through the compress calls
    of include/lzbench_hip.h 3e.
    split_decode=True (zstd only, else ValueError) sizes the decompress temp for the four-kernel split decoder
    (lzh_zstd_ragged_decompress_split_temp_bytes: about 280 KiB per chunk at 128 KiB, several times faster on large
    batches); where there is none (max_chunk_bytes below 16 KiB) the temp stays the small one and every frame
    decodes in the one-wave kernel, as with split_decode=False.
    compact_decode=True (zstd with split_decode=True and no dictionary, else ValueError) runs that decoder in the
    compact temp layout of include/lzbench_hip.h 3g: the temp is sized from max_total_bytes
    (lzh_zstd_ragged_decompress_split_compact_temp_bytes: about twice the batch plus 18 KiB per chunk), so a batch
    of one large chunk among many small ones can use the split decoder; decompress passes max_total_bytes as the
    promised total, and where the sizing call answers 0 the temp stays the small one.
    dictionary=<uint8 tensor of 8 .. 65536 bytes> (lz4 / lz4fast without compact, else ValueError; chunks up to
    4 MiB) shares one LZ4 dictionary among all chunks (include/lzbench_hip.h 3d): compress() writes what
    LZ4_loadDict + LZ4_compress_fast_continue write for each chunk, decompress() is LZ4_decompress_safe_usingDict.
    The tensor is copied once (self.dictionary); small records that share content with it compress several times
    smaller than alone.
    With zstd / zstd_fast the dictionary (8 .. 131072 bytes, raw content; chunks up to 128 KiB; levels 1 and
    -1 .. -5; no compact_scratch, no split_decode, else ValueError) goes through include/lzbench_hip.h 3f: compress()
    writes what ZSTD_compress_usingDict writes for each chunk with the dictionary in a buffer of its own, decompress()
    is ZSTD_decompress_usingDict.  A tensor that begins with zstd's dictionary magic (37 A4 30 EC) is refused with
    ValueError: the reference would read it as a trained dictionary, these calls use the bytes as content.
    zstd_dfast_dict (a name of RaggedCodec's alone; level 3 and a dictionary, else ValueError) is level 3 with that
    dictionary (include/lzbench_hip.h 3h): the limits, the refusals and the decoder of the paragraph above, compress()
    writing what ZSTD_compress_usingDict writes at level 3.  zstd and zstd_dfast keep refusing level 3 with a dictionary.
    lz4frame (level = an LZH_LZ4F_PARAMS value: block-size id 0 | 4 .. 7, the LZ4F_* flags, acceleration << 8) writes one
    LZ4 frame per chunk with independent blocks (include/lzbench_hip.h 3i): the bytes DeviceCodec("lz4frame") writes
    for a chunk size that holds the chunk, a zero-length chunk the 11-byte frame.  A level with LZ4F_LINKED is refused
    with ValueError (linked-block compression is the uniform call's), so are compact, compact_scratch, split_decode,
    compact_decode and a dictionary.  decompress() takes independent and linked frames alike.  Every frame has the
    block slots of max_chunk_bytes: a skewed batch pays for its largest chunk max_chunks times.
    Work is queued on torch's current stream; nothing synchronises with the host.
    """

    def __init__(self, codec: str, max_chunk_bytes: int, max_chunks: int, level: int = 0, device=None,
                 max_total_bytes: Optional[int] = None, compact: bool = False, split_decode: bool = False,
                 compact_scratch: bool = False, dictionary=None, compact_decode: bool = False):
        import torch
        self.torch = torch
        # (zstd_dfast_dict, 3h: a name of RaggedCodec's alone -- level 3 with a dictionary; CODECS does not hold it)
        dfdict = codec == "zstd_dfast_dict"
        if dfdict and dictionary is None:
            raise ValueError("ragged batches: zstd_dfast_dict needs a dictionary (without one: zstd_dfast)")
        if dfdict and level != 3:
            raise ValueError(f"ragged batches: zstd_dfast_dict is level 3 alone (level {level}; 1, -1 .. -5: zstd)")
        self.codec = LZH_CODEC_ZSTD_DFAST if dfdict else CODECS[codec]
        self.level = level if dfdict or codec in _LEVELED else (1 if codec == "lz4" else 0)
        self.max_chunk_bytes, self.max_chunks = max_chunk_bytes, max_chunks
        self.max_total = max_chunks * max_chunk_bytes if max_total_bytes is None else max_total_bytes
        L = lib()
        self.compact = compact
        # (zstd_dfast, level 3: the frames, the decoder, the options and the refusals of zstd; 3e's compress calls)
        dfast = self.codec == LZH_CODEC_ZSTD_DFAST and not dfdict
        self.zstd = self.codec == LZH_CODEC_ZSTD or dfast or dfdict
        if self.zstd and compact:
            raise ValueError("ragged batches: compact=True is the LZ4 / snappy layout; for zstd pass compact_scratch=True")
        if compact_scratch and not self.zstd:
            raise ValueError("ragged batches: compact_scratch is a zstd option (LZ4 / snappy: compact=True)")
        self.compact_scratch = compact_scratch
        if split_decode and not self.zstd:
            raise ValueError("ragged batches: split_decode is a zstd option")
        self.split_decode = split_decode
        if compact_decode and not self.zstd:
            raise ValueError("ragged batches: compact_decode is a zstd option")
        if compact_decode and not split_decode:
            raise ValueError("ragged batches: compact_decode is a layout of the split decoder (pass split_decode=True)")
        if compact_decode and dictionary is not None:
            raise ValueError("ragged batches: a zstd dictionary goes with the one-wave decoder (no compact_decode)")
        self.compact_decode = compact_decode
        lz4f = self.codec == LZH_CODEC_LZ4F
        if lz4f and (compact or dictionary is not None):
            raise ValueError("ragged batches: lz4frame goes with the uniform-slot layout and no dictionary")
        if lz4f and level & LZ4F_LINKED:
            raise ValueError("ragged batches: lz4frame compresses independent blocks (no LZ4F_LINKED in the level)")
        zdict = dictionary is not None and codec in ("zstd", "zstd_fast", "zstd_dfast_dict")
        if zdict and (compact_scratch or split_decode):
            raise ValueError("ragged batches: a zstd dictionary goes with the uniform-slot layout and the one-wave decoder "
                             "(no compact_scratch, no split_decode)")
        if dictionary is not None and not zdict and (codec != "lz4" and codec != "lz4fast" or compact):
            raise ValueError("ragged batches: a dictionary goes with codec lz4 / lz4fast / zstd / zstd_fast and the "
                             "uniform-slot layout (compact=False)")
        # the variant, chosen once: a compress and a decompress row of ragged_calls.RAGGED_CALLS (zstd_dfast decodes with
        # zstd's), and the values their heads and sizing calls pick from by name
        family = ("zstd_dict" if zdict else "zstd_dfast" if dfast else "zstd" if self.zstd
                  else "lz4_dict" if dictionary is not None else "lz4f" if lz4f else "lz")
        # (3h compresses through its own call and decodes through 3f's)
        self._crec = ragged_calls.COMPRESS["zstd_dfast_dict" if dfdict else family, compact or compact_scratch]
        self._drec = ragged_calls.DECOMPRESS["zstd" if dfast else family, compact_decode]
        self._head = dict(codec=self.codec, level=self.level)
        if dictionary is not None:
            nd = self._head["dict_bytes"] = int(dictionary.numel())
        sized = dict(self._head, total=self.max_total, max_chunk_bytes=max_chunk_bytes, nchunks=max_chunks)
        ct = self._crec.temp_bytes(L, **sized)
        dt = self._drec.temp_bytes(L, roomy=split_decode, **sized)
        if ct == 0 or dt == 0:
            if zdict:
                raise ValueError(f"ragged batches: zstd level {self.level} ({'3' if dfdict else '1, -1 .. -5'}) / a dictionary of {nd} bytes "
                                 f"(8 .. 131072) / chunks of {max_chunk_bytes} bytes (up to 131072) are not supported")
            if dictionary is not None:
                raise ValueError(f"ragged batches: a dictionary of {nd} bytes (8 .. 65536) / chunks of {max_chunk_bytes} "
                                 "bytes (up to 4 MiB) are not supported")
            raise ValueError(f"ragged batches: codec {codec} (level {self.level}) / chunks of {max_chunk_bytes} bytes "
                             "are not supported")
        if zdict and bytes(dictionary.reshape(-1)[:4].cpu().numpy().tobytes()) == b"\x37\xa4\x30\xec":   # (read once, here)
            raise ValueError("ragged batches: the dictionary begins with zstd's dictionary magic; trained "
                             "dictionaries are not supported (the bytes would be used as content)")
        self.dev = device or torch.device("cuda", torch.cuda.current_device())
        u8 = dict(dtype=torch.uint8, device=self.dev)
        if dictionary is not None:   # (3d, 3f: the calls read the dictionary with 16 readable bytes after it)
            self.dictionary = torch.zeros(nd + 16, **u8)
            self.dictionary[:nd].copy_(dictionary.reshape(-1))
            self._head["dict"] = self.dictionary.data_ptr()
        if self.zstd:
            self.max_packed = L.lzh_zstd_ragged_max_packed_bytes(self.max_total, max_chunks)
        elif lz4f:
            self.max_packed = L.lzh_lz4f_ragged_max_packed_bytes(self.max_total, max_chunks)
        else:
            self.max_packed = L.lzh_ragged_max_packed_bytes(self.codec, self.max_total, max_chunks)
        self.packed = torch.empty(self.max_packed + 64, **u8)
        self.csizes = torch.empty(max_chunks, dtype=torch.int32, device=self.dev)
        self.offsets = torch.empty(max_chunks + 1, dtype=torch.int64, device=self.dev)
        self.status = torch.empty(max_chunks, dtype=torch.int32, device=self.dev)
        self.ctemp = torch.empty(ct, **u8)
        self.dtemp = torch.empty(dt, **u8)
        self.k = 0

    def _stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def _arrays(self, buf, offsets, sizes, slack):
        """Device arrays (pointers, sizes) of a chunk list over buf, checked on the host."""
        offs = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        szs = np.ascontiguousarray(sizes, dtype=np.int64).reshape(-1)
        if len(offs) != len(szs) or len(offs) > self.max_chunks:
            raise ValueError("ragged batches: offsets / sizes mismatch or more chunks than max_chunks")
        if len(offs) and (offs.min() < 0 or szs.min() < 0 or int((offs + szs).max()) + slack > buf.numel()):
            raise ValueError(f"ragged batches: a chunk (with {slack} bytes of slack) passes the end of the buffer")
        if int(szs.sum()) > self.max_total:
            raise ValueError("ragged batches: more input than max_total_bytes")
        both = np.stack([offs + buf.data_ptr(), szs])
        d = self.torch.from_numpy(both).to(self.dev, non_blocking=False)
        return d, len(offs)

    def compress(self, buf, offsets, sizes) -> None:
        """Compress chunks buf[offsets[i] : offsets[i] + sizes[i]] (each with 16 readable bytes after it inside
        buf) into self.packed / csizes / offsets, as DeviceCodec.compress lays a uniform input out."""
        self.compress_arrays(*self._arrays(buf, offsets, sizes, 16))

    def compress_arrays(self, d, k: int) -> None:
        """compress() on device arrays made before (d: int64 [2, k], chunk addresses and sizes): no host-to-device
        copy, so the call can be captured in a graph."""
        self._in = d   # (kept alive until the next call: the kernels read it asynchronously)
        self.k = k
        self._call(self._crec, in_ptrs=d[0].data_ptr(), in_bytes=d[1].data_ptr(), packed=self.packed.data_ptr(),
                   packed_cap=self.packed.numel(), csizes=self.csizes.data_ptr(), offsets=self.offsets.data_ptr(),
                   temp=self.ctemp.data_ptr(), temp_bytes=self.ctemp.numel())

    def _call(self, rec, **buffers) -> None:
        """rec on the current stream: its head, the batch's shape (the promised total as max_total is now: a caller
        may lower its promise between calls) and the buffers, each argument picked by name."""
        rc = rec(lib(), **self._head, nchunks=self.k, max_chunk_bytes=self.max_chunk_bytes, total=self.max_total,
                 stream=self._stream(), **buffers)
        if rc:
            raise RuntimeError(f"{rec.symbol} failed ({rc})")

    def decompress(self, out_buf, out_offsets, out_sizes, packed=None, csizes=None, offsets=None) -> None:
        """Decode chunk i to out_buf[out_offsets[i] : out_offsets[i] + out_sizes[i]]; self.status[i] = its
        decoded size or a negative verdict.  packed / csizes / offsets default to the last compress call's
        (offsets=None with csizes given: derived on the device)."""
        self.decompress_arrays(*self._arrays(out_buf, out_offsets, out_sizes, 0), packed, csizes, offsets)

    def decompress_arrays(self, d, k: int, packed=None, csizes=None, offsets=None) -> None:
        """decompress() on device arrays made before (d: int64 [2, k], output addresses and sizes)."""
        if csizes is None and offsets is None:
            offsets = self.offsets
        packed = self.packed if packed is None else packed
        csizes = self.csizes if csizes is None else csizes
        self._out = d
        self.k = k
        self._call(self._drec, packed=packed.data_ptr(), packed_readable=packed.numel(), csizes=csizes.data_ptr(),
                   offsets=offsets.data_ptr() if offsets is not None else None, out_ptrs=d[0].data_ptr(),
                   out_bytes=d[1].data_ptr(), status=self.status.data_ptr(), temp=self.dtemp.data_ptr(),
                   temp_bytes=self.dtemp.numel())

    def packed_total(self) -> int:
        return int(self.offsets[self.k].item())
