"""CPU: the argument checks of the four uniform compress calls (include/lzbench_hip.h: lzh_compress_async,
lzh_compress_kernel_stage, lzh_compress_kernel_only, lzh_compress_finish_async), all seven codecs.  Every case of
tests/uniform_fake.py -- one defect, or two at once, which fixes the order of their checks -- returns before any device
call, with the code recorded in tests/golden/uniform_call_verdicts.json from the library of the commit before the
calls were put on one path (csrc/api.cpp: uniform_ok, uniform_call).  The order that file holds:
lzh_compress_async: null pointers, chunk_size 0 and in_readable < n are LZH_EARG; then (but for the memcpy codec) a
short or null temp and a short packed_cap are LZH_ESPACE; then level, chunk size and chunk count are LZH_EARG.  The
other three: LZH_EARG for all but lzh_compress_finish_async's short packed_cap, which comes after its codec."""
import json

import pytest

from uniform_fake import ASYNC, CALLS, CODECS, EARG, ESPACE, FINISH, GOLDEN, MEMCPY, OK, ZSTD, cases, fake_call

with open(GOLDEN) as f:
    VERDICTS = json.load(f)


def test_the_table_covers_every_call_and_codec():
    assert set(VERDICTS) == set(CALLS)
    for call in CALLS:
        assert set(VERDICTS[call]) == {str(c) for c in CODECS}
        for codec in CODECS:
            names = set(VERDICTS[call][str(codec)])
            assert names == set(cases(call, codec)), (call, codec)
            # every defect the call refuses stands alone in it, and in a pair
            assert {"chunk0", "null_d_csizes", "null_d_csizes+chunk0"} <= names
    assert sum(len(t) for c in VERDICTS.values() for t in c.values()) > 1000


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("call", list(CALLS))
def test_verdicts_are_the_recorded_ones(call, codec):
    want = VERDICTS[call][str(codec)]
    got = {name: fake_call(call, codec, name, combo) for name, combo in cases(call, codec).items()}
    assert got == want, {name: (got[name], want[name]) for name in want if got[name] != want[name]}


def test_recorded_order_is_the_documented_one():
    """a few entries of the file read by hand, so that a re-recorded file cannot move the order unnoticed"""
    a, fin = VERDICTS[ASYNC], VERDICTS[FINISH]
    z = a[str(ZSTD)]
    assert z["level0"] == z["chunks_over_u32"] == z["chunk_over_limit"] == EARG
    assert z["temp_short"] == z["temp_null"] == z["cap_short"] == ESPACE
    assert z["level0+temp_short"] == z["level19+cap_short"] == z["chunks_over_u32+temp_null"] == ESPACE
    assert z["short_readable+temp_short"] == z["null_d_packed+cap_short"] == z["chunk0+temp_null"] == EARG
    m = a[str(MEMCPY)]
    assert m["empty"] == m["empty+null_d_in+temp_null"] == OK and m["cap_short"] == m["temp_null+cap_short"] == ESPACE
    assert fin[str(ZSTD)]["cap_short"] == ESPACE and fin[str(MEMCPY)]["cap_short"] == EARG
    assert fin[str(ZSTD)]["null_d_offsets+cap_short"] == EARG

