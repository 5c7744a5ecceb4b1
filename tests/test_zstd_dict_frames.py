"""CPU: the hand-built frames of the zstd dictionary decoder (tests/zstd_dict_frames.py): the walker ends on each,
the reference build's ZSTD_decompress_usingDict -- where it is present -- gives the model's status and bytes (the
repeat-offset rules and the header variants take their truth from it), and the classifier's events: the hand frames
reach every one, and a printed table says which of them the encoder-made frames of the round-trip tests reach
(tests/test_gpu_zstd_dict.py runs the frames on the GPU)."""

import numpy as np
import pytest

import lzbench_amd as L
import zstd_census as Z
import zstd_dict_frames as F
import zstd_dict_inputs as I
import zstd_dict_ref as R

NAMES = list(F.FRAMES)


@pytest.mark.parametrize("name", NAMES)
def test_walker_ends_on_the_frame(name):
    _, frame, content, _ = next(f for f in F.frames() if f[0] == name)
    c, blocks, fcs = Z.walk(frame, reserved_ok=name.startswith("reserved"))
    assert fcs == len(content) and c["block/cmp"] == len(blocks) >= 1
    assert c["LL/rle"] == c["OF/rle"] == c["ML/rle"] == len(blocks)
    if name.startswith("reserved"):
        with pytest.raises(Z.CensusError, match="reserved table-mode bits"):
            Z.walk(frame)


@pytest.mark.parametrize("name", NAMES)
def test_reference_gives_the_models_status_and_bytes(name):
    R.need()
    d = F.dictionary()
    _, frame, content, _ = next(f for f in F.frames() if f[0] == name)
    want = F.expected(name, d)
    assert want == ((len(content), content) if name != "dict-id-nonzero" else (-1, b""))
    assert R.decompress(d, frame, len(content)) == want, f"{name}: the reference disagrees with the model"
    for other, cut in F.REJECTS:
        if other == name:
            short = d[cut:]
            assert F.expected(name, short)[0] == -1
            assert R.decompress(short, frame, len(content))[0] < 0, f"{name}: accepted with a shorter dictionary"
    if name in F.NEEDS_NO_DICTIONARY:
        assert R.decompress(np.zeros(0, np.uint8), frame, len(content)) == want


def test_model_rules():
    """the repeat offsets, each against bytes worked out here"""
    d = F.dictionary()
    db = d.tobytes()
    _, c, t = F.build("initial-rep1", d)
    assert t[0][:4] == (0, 0, 30, 4) and t[0].rep and c[:30] == (db[-4:] * 8)[:30]
    _, c, t = F.build("initial-rep2", d)
    assert t[0].off == 8 and c[:30] == (db[-8:] * 4)[:30]
    _, c, t = F.build("initial-rep0-minus-1", d)
    assert t[0].off == 1 and c[:30] == db[-1:] * 30
    _, c, t = F.build("rep-across-blocks", d)
    assert [e.off for e in t if e.ml] == [300, 300, 300] and [e.rep for e in t if e.ml] == [False, True, True]
    assert c[64:164] == db[-236:-136] and c[234:300] == db[-66:] and c[300:344] == c[:44] and c[408:507] == c[108:207]
    _, c, t = F.build("dict-first-byte", d)
    assert c[7:7 + F.ND] == db
    with pytest.raises(F.Reject):
        F.build("dict-first-byte", d[1:])
    for name, frame, content, _ in F.frames():
        assert 9 <= len(frame) and len(content) <= 8192, name


# what each frame is for: the events its dictionary sequences must show
FRAME_EVENTS = {
    "whole-short": {"dict/whole"},
    "whole-multi-round": {"dict/whole", "dict/copy>64"},
    "whole-wrap": {"dict/whole", "dict/copy>window"},
    "dict-first-byte": {"dict/first-byte", "dict/whole", "dict/copy>window"},
    "straddle-period-2": {"dict/straddle/period"},
    "straddle-period-1": {"dict/straddle/period"},
    "straddle-period-37": {"dict/straddle/period"},
    "straddle-window": {"dict/straddle/window"},
    "straddle-far": {"dict/straddle/far", "dict/straddle/far-overlap", "dict/after-bulk"},
    "straddle-far-reach": {"dict/straddle/far"},
    "after-bulk-literals": {"dict/after-bulk", "dict/straddle/far"},
    "group-dict-group": {"dict/after-group", "dict/before-group", "dict/whole"},
    "group-straddle-group": {"dict/after-group", "dict/before-group", "dict/straddle/window"},
    "initial-rep1": {"dict/rep", "dict/straddle/period"},
    "initial-rep2": {"dict/rep", "dict/straddle/period"},
    "initial-rep0-minus-1": {"dict/rep", "dict/straddle/period"},
    "rep-across-blocks": {"dict/rep", "dict/whole", "dict/straddle/window"},
    "reserved-bit0-plain": set(),
    "reserved-bit1-dict": {"dict/whole"},
    "dict-id-zero": {"dict/whole"},
    "dict-id-nonzero": {"dict/whole"},
    "window-descriptor": {"dict/straddle/window"},
    "long-literals-then-dict": {"dict/long-literals", "dict/straddle/window"},
}


@pytest.mark.parametrize("name", NAMES)
def test_frame_reaches_its_events(name):
    _, _, _, trace = next(f for f in F.frames() if f[0] == name)
    ev = F.events(trace, F.ND)
    assert FRAME_EVENTS[name] <= ev, (name, sorted(ev))
    if name in F.NEEDS_NO_DICTIONARY:
        assert not ev
    if name == "straddle-far-reach":
        assert "dict/after-bulk" not in ev
    if name == "rep-across-blocks":              # the last use of rep0 has become an offset into the output
        assert [bool(n) for _, n in F.classify(trace, F.ND)] == [True, True] and sum(1 for e in trace if e.ml) == 3


def test_hand_frames_reach_every_event():
    u = set()
    for name, _, _, trace in F.accepting():
        u |= F.events(trace, F.ND)
    assert u == set(F.EVENTS), sorted(set(F.EVENTS) - u)


def _walk(level, d, c):
    dd = np.concatenate([d, np.zeros(16, np.uint8)])
    cc = np.concatenate([c, np.zeros(16, np.uint8)])
    cap = len(c) // 4 + 16
    s = np.zeros(3 * cap, np.uint32)
    k = L.lib().lzh_debug_zstd_dict_parse(level, dd.ctypes.data, len(d), cc.ctypes.data, len(c), s.ctypes.data, cap)
    assert 0 <= k <= cap
    return s[: 3 * k].reshape(-1, 3).astype(np.int64)


def test_events_the_round_trip_tests_reach():
    """Information, no assertion on the table: the events in the frames the encoder writes for the round-trip tests'
    inputs (the host walk's sequences are the frame's), per source."""
    rows = {}
    for level in I.LEVELS:
        u = set()
        for name, (d, c) in I.constructed().items():
            u |= F.events(F.trace_of_walk(_walk(level, d, c), len(c)), len(d))
        rows[f"constructed, level {level}"] = u
        u = set()
        for _, kind, d in I.dictionaries():
            for _, c in I.chunks(kind, len(d)):
                u |= F.events(F.trace_of_walk(_walk(level, d, c), len(c)), len(d))
        rows[f"matrix, level {level}"] = u
    hand = set()
    for _, _, _, trace in F.accepting():
        hand |= F.events(trace, F.ND)
    rows["hand frames"] = hand
    print()
    print(f"{'event':28s}" + "".join(f"{k:>24s}" for k in rows))
    for ev in F.EVENTS:
        print(f"{ev:28s}" + "".join(f"{'yes' if ev in u else '-':>24s}" for u in rows.values()))
    assert hand == set(F.EVENTS)
