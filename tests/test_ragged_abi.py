"""CPU: the ragged-batch calls of include/lzbench_hip.h 3b without a device -- sizing functions (the calls'
argument checks: tests/test_ragged_calls_abi.py), and the invariance of the uniform kernels' code hashes."""
import os
import shutil
import subprocess

import pytest

import lzbench_amd as L
from lzbench_amd.kernel_hash import kernel_hashes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LZ4, SNAPPY = L.LZH_CODEC_LZ4, L.LZH_CODEC_SNAPPY


@pytest.mark.parametrize("codec", [LZ4, SNAPPY])
def test_sizing_functions(codec):
    lib = L.lib()
    for f in (lib.lzh_ragged_compress_temp_bytes, lib.lzh_ragged_decompress_temp_bytes):
        for maxb in (0, 1, 4099, 65536, 65537, 200000, 16 << 20):
            prev = 0
            for k in (0, 1, 2, 255, 256, 257, 1000, 16384):
                v = f(codec, maxb, k)
                assert v >= prev and v > 0, (maxb, k)
                prev = v
        for k in (1, 7, 1000):
            prev = 0
            for maxb in (0, 1, 15, 4099, 65535, 65536, 65537, 131072, 131073, 1 << 20, 16 << 20):
                v = f(codec, maxb, k)
                assert v >= prev, (maxb, k)
                prev = v
    for k in (0, 1, 16, 1000):
        prev = 0
        for n in (0, 1, 254, 255, 256, 65536, 1 << 20, 1 << 30):
            v = lib.lzh_ragged_max_packed_bytes(codec, n, k)
            assert v >= prev and v >= n
            prev = v
    for n in (0, 1, 65536, 1 << 20):
        prev = 0
        for k in (0, 1, 2, 1000):
            v = lib.lzh_ragged_max_packed_bytes(codec, n, k)
            assert v >= prev
            prev = v
        assert lib.lzh_ragged_max_packed_bytes(codec, n, 1) >= lib.lzh_max_packed_bytes(codec, n, max(n, 1))
    for maxb in (0, 13, 65536, 200000, 16 << 20):
        for k in (1, 3, 1000):
            assert lib.lzh_ragged_compress_temp_bytes(codec, maxb, k) >= k * lib.lzh_stage_stride(codec, maxb)


@pytest.fixture(scope="module")
def parent_library(tmp_path_factory):
    """liblzbench_hip.so built from the parent commit in a temporary worktree."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: cannot build the parent commit")
    if shutil.which("git") is None or not os.path.isdir(os.path.join(ROOT, ".git")):
        pytest.skip("not a git checkout: no parent commit to build")
    if subprocess.run(["git", "-C", ROOT, "rev-parse", "--verify", "-q", "HEAD~1"], capture_output=True).returncode:
        pytest.skip("no parent commit")
    # the feature's own commit: HEAD when the tree is clean, else the uncommitted tree sits on top of its parent
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--untracked-files=no"], capture_output=True,
                           text=True).stdout.strip()
    rev = "HEAD" if dirty else "HEAD~1"
    wt = str(tmp_path_factory.mktemp("parent") / "wt")
    subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", wt, rev], check=True, capture_output=True)
    try:
        subprocess.run(["make", "-C", os.path.join(wt, "lzbench_amd", "csrc"), "-j8", "../liblzbench_hip.so"],
                       check=True, capture_output=True)
        yield os.path.join(wt, "lzbench_amd", "liblzbench_hip.so")
    finally:
        subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", wt], capture_output=True)


# Kernels a commit changed on purpose, by the hash they had in that commit's parent: the exception is meant only against
# that very parent build, so that every later commit is held to all hashes again.  The code cannot tell one parent from
# another -- an entry excuses its kernel for as long as the kernel keeps that hash -- so the entries are removed by the
# commit after the one that added them, and the dictionary is empty unless the last commit changed a kernel.  (An
# out-of-line callee such as lz4v3::compress_chunk is hashed into every kernel of its code object: changing it moves
# the kernels of lz4c_hip.hip, ragged_hip.hip and ragged_compact_hip.hip together.)
CHANGED_ON_PURPOSE = {}


def test_uniform_kernel_hashes_unchanged(parent_library):
    """profiles/traffic*.json and bench.py's traffic figure are keyed to kernel code hashes: every kernel of
    the parent build keeps its hash, but for the ones a commit changed on purpose (CHANGED_ON_PURPOSE)."""
    old = kernel_hashes(parent_library)
    new = kernel_hashes(L.LIB_PATH)
    assert old, "no kernels found in the parent build"
    changed = {k: (v, new.get(k)) for k, v in old.items() if new.get(k) != v and CHANGED_ON_PURPOSE.get(k) != v}
    assert not changed, f"kernels whose code changed: {changed}"
    assert all(k in new for k in old), "a kernel of the parent build is gone"
