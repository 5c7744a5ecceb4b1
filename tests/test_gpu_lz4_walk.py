"""LZ4 parse, the run batch's chain walk (lz4c.h, lz4v3::compress_chunk): a run batch resolves every sequence that
starts in its 64 positions by walking the per-lane links from member to member.  The inputs here are built so that
the walk meets chains of every length from 1 to 16, exits of every kind (the chain leaves the batch, a long match, the
parse's end) at odd and at even chain positions, batches with and without slot collisions and re-resolve rounds; each
input's property is checked on the CPU first, from the checker's own sequence list and a model of how the kernel
lays its batches over it (batches_of), so a generator that stops producing its case fails instead of passing empty.
Every case then compares packed bytes and compr_sizes with the CPU checker and round-trips through the decoder.
Run with -m gpu."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import lzc_census as Z
import oracle_lib as O
import lzbench_amd as L
from gpu_batches import torch_cuda
from test_gpu_lz4_parse_tail import _hash13, no_collision_chunk

pytestmark = pytest.mark.gpu

WAVE = 64
LONG = 24          # a match of 4 + 20 bytes or more from its probe position leaves the candidate window (slow_count)


# ---- the CPU side: sequences of a chunk, and the run batches the kernel lays over them ---------------------------------
def stream_sequences(stream, n):
    """[(match start, match end)] of one chunk's LZ4 block"""
    seqs, ip, pos = [], 0, 0
    while ip < len(stream):
        t = stream[ip]
        ip += 1
        lit = t >> 4
        if lit == 15:
            while True:
                b = stream[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        ip += lit
        pos += lit
        if ip >= len(stream):
            break
        ip += 2
        ml = (t & 15) + 4
        if ml == 19:
            while True:
                b = stream[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        seqs.append((pos, pos + ml))
        pos += ml
    assert pos == n
    return seqs


def sequences(data):
    """[(probe position, match end)] of one chunk under 64 KiB at acceleration 1, and the census of its parse.  The
    kernel's members are probe positions (where the hash hit, before the match is extended backwards), which the
    stream does not hold: the parse of lz4.c:851-1240 (byU16) is run again here with its table, and must give the
    checker's own sequence list (match start, match end)."""
    data = np.ascontiguousarray(data)
    stream, census = Z.lz4(data)
    n = len(data)
    assert 13 <= n < 65547
    by = data.tobytes() + bytes(8)
    w32 = lambda i: int.from_bytes(by[i:i + 4], "little")
    table = {}
    probes, starts = [], []
    anchor, ip = 0, 1
    mfl1, mlimit = n - 12 + 1, n - 5
    table[_hash13(w32(0))] = 0
    done = False
    while not done:
        fwd, step, nb = ip, 1, 64
        while True:
            ip = fwd
            fwd += step
            step = nb >> 6
            nb += 1
            if fwd > mfl1:
                done = True
                break
            h = _hash13(w32(ip))
            m = table.get(h, 0)
            table[h] = ip
            if w32(m) == w32(ip):
                break
        if done:
            break
        probe = ip
        while ip > anchor and m > 0 and by[ip - 1] == by[m - 1]:
            ip, m = ip - 1, m - 1
        while True:
            ml = 4
            while ip + ml < mlimit and by[ip + ml] == by[m + ml]:
                ml += 1
            probes.append((probe, ip + ml))
            starts.append((ip, ip + ml))
            ip += ml
            anchor = ip
            if ip >= mfl1:
                done = True
                break
            table[_hash13(w32(ip - 2))] = ip - 2
            h = _hash13(w32(ip))
            m = table.get(h, 0)
            table[h] = ip
            if w32(m) != w32(ip):
                ip += 1
                break
            probe = ip
    assert starts == stream_sequences(stream, n), "the parse restated here is not the checker's"
    assert len(probes) == census["lz4/sequences"]
    return probes, census


def batches_of(seqs):
    """The run batches of lz4v3::compress_chunk at acceleration 1 over one chunk's sequences (lz4c.h, the parse state
    base / q / qlim / pins): a list of member lists [(chain position, start lane, end lane)], an empty list for a
    batch whose first segment finds nothing.  A search of 64 probes without a hit goes to stride batches, which find
    the next sequence alone and hand back to run batches at its end - 2 (not listed)."""
    out, i = [], 0
    base, q, qlim = 1, 1, 64
    while i < len(seqs):
        hi0 = min(qlim - base, WAVE - 1)
        members = []
        if seqs[i][0] <= base + hi0:
            while i < len(seqs) and seqs[i][0] <= base + WAVE - 1:
                assert seqs[i][0] >= base
                members.append((len(members), seqs[i][0] - base, seqs[i][1] - base))
                i += 1
                if members[-1][2] >= WAVE:
                    break
        out.append(members)
        if members:
            ip, el = base + members[-1][2], members[-1][2]
            qlim = ip + 64
            if el < WAVE:
                base = q = base + WAVE
            else:
                q = ip
                base = ip - 2 if el - 2 >= WAVE else ip
        elif hi0 == qlim - base:            # 64 probes done: stride batches up to the next sequence
            if i == len(seqs):
                break
            ip = seqs[i][1]
            i += 1
            base, q, qlim = ip - 2, ip, ip + 64
        else:
            base = q = base + hi0 + 1
    return out


def shape_census(data):
    """what the walk meets in one chunk: Counter of ("chain", length), ("leaves", parity of the last member's chain
    position), ("long", chain position) for a long match, ("stays", parity) for a chain that ends inside its batch"""
    seqs, census = sequences(data)
    c = Counter()
    for members in batches_of(seqs):
        if not members:
            c["empty"] += 1
            continue
        c[("chain", len(members))] += 1
        k, start, end = members[-1]
        c[("leaves" if end >= WAVE else "stays", k & 1)] += 1
        for k, start, end in members:
            if end - start >= LONG:
                c[("long", min(k, 3))] += 1
    return c, seqs, census


# ---- inputs ------------------------------------------------------------------------------------------------------------
def pieces_chunk(n, seed, lens=(4,), gap_p=0.0, gaps=(8, 40), long_p=0.0, tail=None):
    """64 distinct bytes, then copies of 4- to 7-byte pieces of them laid back to back (every piece a match that the
    re-test at the previous match's end finds: members at the pieces' stride), now and then a gap of fresh bytes (a
    search: shorter chains) or a copy of 25 to 60 bytes (a long match); tail: the last `tail` bytes are fresh"""
    rng = np.random.default_rng(seed)
    head = rng.permutation(256)[:64].astype(np.uint8)
    out = [head]
    have = 64
    while have < n:
        r = rng.random()
        if r < gap_p:
            piece = rng.integers(0, 256, int(rng.integers(gaps[0], gaps[1] + 1))).astype(np.uint8)
        elif r < gap_p + long_p:
            k = int(rng.integers(25, 61))
            s = int(rng.integers(1, 64 - k + 1))
            piece = head[s:s + k]
        else:
            k = int(lens[rng.integers(0, len(lens))])
            s = int(rng.integers(1, 64 - k + 1))
            piece = head[s:s + k]
        out.append(piece)
        have += len(piece)
    d = np.concatenate(out)[:n].copy()
    if tail:
        d[n - tail:] = rng.integers(0, 256, tail).astype(np.uint8)
    return d


def dense_no_collision_chunk(n, seed):
    """as no_collision_chunk (no two of any 64 consecutive positions share a table slot), with short copies one after
    the other: long chains in batches without a collision"""
    rng = np.random.default_rng(seed)
    out = bytearray(n)
    slots, recent = [], {}
    src, left = 0, 0
    fresh = rng.integers(0, 256, size=(n, 6))
    plan = rng.integers(0, 1 << 30, size=(n, 2))
    for i in range(n):
        if left == 0 and i > 200 and plan[i, 0] % 2 == 0:
            src, left = int(plan[i, 1] % (i - 100)), 4 + int(plan[i, 0] >> 8) % 5
        cands = ([out[src]] if left else []) + [int(b) for b in fresh[i]]
        took = None
        for j, b in enumerate(cands):
            if i < 3:
                took = b
                break
            h = _hash13(out[i - 3] | out[i - 2] << 8 | out[i - 1] << 16 | b << 24)
            if h not in recent:
                took, hh = b, h
                if not (left and j == 0):
                    left = 0
                break
        assert took is not None
        out[i] = took
        if left:
            src, left = src + 1, left - 1
        if i >= 3:
            slots.append(hh)
            recent[hh] = 1
            if len(slots) > 63:
                del recent[slots[-64]]
    return np.frombuffer(bytes(out), np.uint8).copy()


def shared_slots(data):
    """positions whose 4-gram's byU16 slot is also the slot of one of the 63 positions before it"""
    w = data[:-3].astype(np.uint64) | data[1:-2].astype(np.uint64) << 8 | data[2:-1].astype(np.uint64) << 16 \
        | data[3:].astype(np.uint64) << 24
    h = _hash13(w)
    return sum(int((h[d:] == h[:-d]).sum()) for d in range(1, 64))


# ---- the GPU side ------------------------------------------------------------------------------------------------------
def _check(torch, data, chunk, codec="lz4", level=1):
    n = len(data)
    d_in = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(torch.from_numpy(data))
    dc = L.DeviceCodec(codec, n, chunk, level=level)
    dc.compress(d_in)
    dc.decompress()
    torch.cuda.synchronize()
    exp_packed, exp_cs = O.compress_chunks(data, codec, chunk, level, use_ref=O.have_ref())
    cs = dc.csizes.cpu().numpy().astype(np.uint64)
    if not (len(cs) == len(exp_cs) and (cs == exp_cs).all()):
        return f"compr_sizes {cs.tolist()} != {exp_cs.tolist()}"
    total = dc.packed_total()
    if total != len(exp_packed) or not (dc.packed[:total].cpu().numpy() == exp_packed).all():
        return "packed bytes differ"
    if not (dc.status.cpu().numpy() >= 0).all() or not (dc.out[:n].cpu().numpy() == data).all():
        return "round trip failed"
    return None


def _check_all(torch, data, chunk):
    """lz4 and lz4fast at accelerations 2, 3 and 7 on the same bytes"""
    bad = [(codec, level, why) for codec, level in (("lz4", 1), ("lz4fast", 2), ("lz4fast", 3), ("lz4fast", 7))
           for why in [_check(torch, data, chunk, codec, level)] if why]
    assert not bad, bad


def kernel_counters(torch, data):
    """the parse kernel's own event counters over one chunk (lzh_debug_lz4_stats, acceleration 1)"""
    f = L.lib().lzh_debug_lz4_stats
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(data)
    dc = L.DeviceCodec("lz4", n, n)
    d_in = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    d_in[:n].copy_(torch.from_numpy(data))
    st = torch.zeros(32, dtype=torch.int64, device="cuda")
    assert f(d_in.data_ptr(), n, d_in.numel(), n, 1, dc.ctemp.data_ptr(), dc.csizes.data_ptr(), st.data_ptr(),
             torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    v = st.cpu().tolist()
    return {"collision_batches": v[1], "extra_rounds": v[2], "sequences": v[3], "count_slow": v[6], "walk_steps": v[7],
            "resolve_rounds": v[8]}


# chains of every length: pieces of 4 bytes give 16 members a batch, longer and mixed pieces the lengths below, gaps
# the short ones
CHAIN_INPUTS = {
    "stride4": lambda: pieces_chunk(4096, 1),
    "stride5": lambda: pieces_chunk(4096, 2, lens=(5,)),
    "stride4to7": lambda: pieces_chunk(4096, 3, lens=(4, 5, 6, 7)),
    "gaps": lambda: pieces_chunk(4096, 4, lens=(4, 5, 6, 7), gap_p=0.25),
    "long": lambda: pieces_chunk(4096, 5, lens=(4, 5, 6, 7), gap_p=0.1, long_p=0.2),
}


def test_chain_lengths_and_exits(torch_cuda):
    """chains of 1 .. 16 members; the chain leaves its batch after a member at an even and at an odd chain position
    (the first and the second hop of a two-member walk step), ends inside it likewise; a long match alone, as the
    first, the second and the third member"""
    seen = Counter()
    for name, make in CHAIN_INPUTS.items():
        data = make()
        c, seqs, census = shape_census(data)
        seen.update(c)
        _check_all(torch_cuda, data, len(data))
    for k in range(1, 17):
        assert seen[("chain", k)], (k, sorted(x for x in seen if x != "empty" and x[0] == "chain"))
    for kind in ("leaves", "stays"):
        assert seen[(kind, 0)] and seen[(kind, 1)], (kind, seen)
    for k in (0, 1, 2):
        assert seen[("long", k)], (k, seen)
    alone = False
    for name in ("long",):
        seqs, _ = sequences(CHAIN_INPUTS[name]())
        alone = alone or any(len(m) == 1 and m[0][2] - m[0][1] >= LONG for m in batches_of(seqs))
    assert alone, "no batch whose only member is a long match"


def test_kernel_counts_the_model_s_batches(torch_cuda):
    """the model of the batches is the kernel's: every run batch resolves once plus once per re-resolve round, and the
    walk takes at least one step per batch with a member and at most one per member and round"""
    for name, make in CHAIN_INPUTS.items():
        data = make()
        seqs, census = sequences(data)
        b = batches_of(seqs)
        k = kernel_counters(torch_cuda, data)
        assert k["sequences"] == len(seqs), (name, k)
        assert k["resolve_rounds"] - k["extra_rounds"] == len(b), (name, k, len(b))
        with_members = sum(1 for m in b if m)
        in_run = sum(len(m) for m in b)
        assert with_members <= k["walk_steps"] <= (in_run + WAVE * k["extra_rounds"]), (name, k, with_members, in_run)


@pytest.mark.parametrize("n", [64, 100, 1000, 4096])
def test_sizes_and_three_chunks(torch_cuda, n):
    """one to three chunks of 64 B .. 4 KiB (the last one short)"""
    data = np.concatenate([pieces_chunk(n, 10, lens=(4, 5)), pieces_chunk(n, 11, lens=(4, 6, 7), gap_p=0.2),
                           pieces_chunk(max(n - 25, 13), 12, long_p=0.1)])
    for k in (1, 2, 3):
        _check_all(torch_cuda, data[:min(k * n, len(data))], n)


@pytest.mark.parametrize("n", [65536, 65547])
def test_full_chunk_byu16_and_byu32(torch_cuda, n):
    """64 KiB (byU16) and 65 547 bytes (the byU32 instantiation) of mixed pieces, gaps and long copies"""
    data = pieces_chunk(n, 20 + (n & 1), lens=(4, 5, 6, 7), gap_p=0.15, long_p=0.05)
    census = Z.lz4(data)[1]
    assert census["lz4/table/byU32" if n >= 65547 else "lz4/table/byU16"]
    assert census["lz4/retest-chain>=8"] > 20 and census["lz4/count/21-275"] > 100 and census["lz4/hit/search"] > 100
    _check_all(torch_cuda, data, n)


def test_parse_ends_inside_a_pair(torch_cuda):
    """the tail body: chunks of 64 + 24 bytes, eight less to eight more, of dense pieces, so the parse's last match
    ends at or past mflimit as a member at an even and at an odd chain position, or (fresh last bytes) the search
    runs out"""
    ends = Counter()
    for n in range(64 + 24 - 8, 64 + 24 + 9):
        for seed, lens, tail in ((30, (4,), None), (31, (4, 5), None), (32, (5, 6, 7), 14)):
            data = pieces_chunk(n, seed, lens=lens, tail=tail)
            seqs, census = sequences(data)
            b = batches_of(seqs)
            if census["lz4/end/match-at-mflimit"]:
                last = [m for m in b if m][-1][-1]
                ends[("match", last[0] & 1)] += 1
            else:
                ends["search"] += census["lz4/end/search-ran-out"]
            _check_all(torch_cuda, data, n)
    assert ends[("match", 0)] and ends[("match", 1)] and ends["search"], ends


def test_re_resolve_rounds(torch_cuda):
    """4-grams repeated inside 64 positions: lanes share slots, and the resolve takes more than one round (counted by
    the kernel: extra_rounds).  The pieces come from 61 4-grams, so every batch of a dense input repeats some, before,
    between and on its members.  Every round walks the chain from the batch's first member (resuming after a kept
    prefix was measured slower and is not in the kernel), so where the first corrected lane lies relative to the
    members selects no code path and is not pinned case by case."""
    for name in ("stride4", "stride4to7", "gaps"):
        data = CHAIN_INPUTS[name]()
        assert shared_slots(data) >= len(data) // WAVE     # one a batch or more
        k = kernel_counters(torch_cuda, data)
        assert k["collision_batches"] > 0 and k["extra_rounds"] > 0, (name, k)
        assert k["resolve_rounds"] > k["collision_batches"], (name, k)


@pytest.mark.parametrize("make", [no_collision_chunk, dense_no_collision_chunk], ids=["sparse", "dense"])
def test_collision_free_batches(torch_cuda, make):
    """no two of 64 consecutive positions share a slot: every batch resolves in the collision-free body"""
    data = make(4096, 41)
    assert shared_slots(data) == 0
    c, seqs, census = shape_census(data)
    if make is dense_no_collision_chunk:
        assert max(x[1] for x in c if x != "empty" and x[0] == "chain") >= 4, c
    k = kernel_counters(torch_cuda, data)
    assert k["collision_batches"] == 0 and k["extra_rounds"] == 0 and k["sequences"] == len(seqs), k
    _check_all(torch_cuda, data, len(data))
    _check_all(torch_cuda, np.concatenate([data, make(4096 - 25, 42)]), 4096)
