"""The device module where the production geometry differs from what the other GPU tests build:
lane offsets past 2^31 and 2^32 from the arena base, PartHasher launches over many 1 GiB slots,
a streamed-verify chunk larger than the staging slot, unreadable storage on the GPU paths, and
the sha1_pieces arms that only the kernel benches launch. Every comparison is bit-exact against
hashlib on seeded data; the seed is in the test id.
"""
from __future__ import annotations

import functools
import hashlib
import os
import random
import threading
import time

import pytest

from test_gpu_lane_tables import (KERNELS, LONG, _flip_offset, ragged_table, ref,
                                  tails_table)

GiB = 1 << 30
B31, B32 = 1 << 31, 1 << 32


# --------------------------------------------------- 1. lane tables high in the device buffer
# name -> (seed, builder, base, the 2^k boundary the base is chosen for)
# `tails` is 192 lanes at a stride of 256 and `base` a multiple of 256, so with the bases below
# the boundary falls on the start of lane 96: lanes on both sides of it, none across it. The
# same table moved up 128 bytes has lane i >= 128 reach into the next 256 bytes: with the
# boundary at the start of its 161st stride, lane 160 (two whole blocks + 32 bytes) lies across.
# ragged-long-last at 2^32 - 65536 has a short lane across the boundary (its 1,026-block lane
# starts ~157 KB into the table); with the long lane first that lane starts at the base, runs
# 1,024 blocks up to the boundary and has its 57-byte tail (two padding blocks) above it.
HIGH = {
    "tails-2^31": (501, tails_table, B31 - 24576, B31),
    "tails-2^32": (502, tails_table, B32 - 24576, B32),
    "tails+128-2^31": (503, functools.partial(tails_table, 256, 128), B31 - 161 * 256, B31),
    "tails+128-2^32": (504, functools.partial(tails_table, 256, 128), B32 - 161 * 256, B32),
    "ragged-long-last-2^32": (505, ragged_table, B32 - 65536, B32),
    "ragged-long-first-2^32": (506, functools.partial(ragged_table, True), B32 - 65536, B32),
    "ragged-long-last-5GiB": (507, ragged_table, 5 * GiB, B32),
    "tails-5GiB": (508, tails_table, 5 * GiB, B32),
}
ON_A_LANE_START = ("tails-2^31", "tails-2^32")
WHOLLY_ABOVE = ("ragged-long-last-5GiB", "tails-5GiB")


@functools.lru_cache(maxsize=None)
def high_table(name):
    """(data, offsets, lengths, hashlib digests, base): built once, immutable."""
    seed, build, base, _ = HIGH[name]
    offs, lens, size = build()
    data = random.Random(seed).randbytes(size)
    want = tuple(hashlib.sha1(data[o:o + n]).digest() for o, n in zip(offs, lens))
    return data, tuple(offs), tuple(lens), want, base


def sides(offs, lens, base, boundary):
    """Lanes whose bytes lie (entirely below, across, entirely above) the boundary."""
    below = [i for i, (o, n) in enumerate(zip(offs, lens)) if n and base + o + n <= boundary]
    across = [i for i, (o, n) in enumerate(zip(offs, lens)) if base + o < boundary < base + o + n]
    above = [i for i, (o, n) in enumerate(zip(offs, lens)) if n and base + o >= boundary]
    return below, across, above


def test_high_tables_sit_where_they_claim():
    assert tails_table()[2] == 49152
    for name, (seed, build, base, boundary) in HIGH.items():
        offs, lens, size = build()
        assert base % 256 == 0 and 0 <= base <= 8 * GiB, name
        assert all(o % 16 == 0 for o in offs), name
        below, across, above = sides(offs, lens, base, boundary)
        assert len(below) + len(across) + len(above) == sum(1 for n in lens if n), name
        if name in WHOLLY_ABOVE:
            assert base >= 5 * GiB and not below and not across and above, name
            continue
        assert base < boundary < base + size, name          # the boundary is inside the table
        # (with the long lane first nothing lies below it: that table is here for the lane across)
        assert above and (below or name == "ragged-long-first-2^32"), name
        if name in ON_A_LANE_START:
            # base and stride are multiples of 256: no lane of this table can lie across
            assert not across and boundary - base == offs[96] == 24576, name
        else:
            assert across, name
    _, lens, _ = tails_table(256, 128)
    _, across, _ = sides(*tails_table(256, 128)[:2], HIGH["tails+128-2^32"][2], B32)
    assert across == [160] and lens[160] == 2 * 64 + 32
    offs, lens, _ = ragged_table()
    _, across, _ = sides(offs, lens, B32 - 65536, B32)
    assert len(across) == 1 and lens[across[0]] != LONG and lens[across[0]] > 64
    offs, lens, _ = ragged_table(True)
    assert sides(offs, lens, B32 - 65536, B32)[1] == [0] and lens[0] == LONG
    assert offs[0] + (LONG & ~63) == 65536                  # only its tail is above 2^32


# ------------------------------------------------ 2. PartHasher: eight 1 GiB slots, 64 lanes
SLOT, LANES, SLOTS = GiB, 64, 8
GATE = 16 << 20
# (piece length, pieces, length of the last piece); in submission order
ALIGNED = [
    (16, 64, 16),
    (48, 40, 48), (64, 24, 63),              # two parts in one slot: the second at lane0 = 40
    (1008, 64, 64 + 56),                     # last piece 56 bytes past a block: two padding blocks
    (16384, 64, 16384),
    (65552, 64, 65552),
    (4096, 64, 5),
    (16384, 40, 55), (16, 24, 1),
    (16384, 3, 56),                          # every slot taken: waits for a free one
]
MIXED = list(ALIGNED)
MIXED[1] = (999, 40, 57)                     # byte loads
MIXED[3] = (1000, 64, 64 + 56)               # dword loads in sha1_pieces, byte loads here
# the slots of the launch that follows the gate, by index into the lists above
CLAIMED = [[0], [1, 2], [3], [4], [5], [6], [7, 8]]


def part_bytes(part):
    piece, n, last = part
    return piece * (n - 1) + last


def pack(parts, slot_bytes=SLOT, max_lanes=LANES):
    """The dispatcher's packing rule (part_dispatch.h): a part starts at the slot's fill rounded
    up to 256, and the open slot closes when lanes + np > max_lanes or off + len > slot_bytes.
    -> per slot a list of (part index, offset in the slot, first lane)."""
    slots, used, lanes = [[]], 0, 0
    for k, part in enumerate(parts):
        off = (used + 255) & ~255
        if slots[-1] and (lanes + part[1] > max_lanes or off + part_bytes(part) > slot_bytes):
            slots.append([])
            used = lanes = off = 0
        slots[-1].append((k, off, lanes))
        lanes += part[1]
        used = off + part_bytes(part)
    return slots


def test_follower_parts_fill_the_slots_they_claim():
    assert {16, 48, 64, 1008, 16384, 65552, 4096} == {p[0] for p in ALIGNED}
    assert all(p[0] % 16 == 0 for p in ALIGNED)
    assert sorted(p[0] for p in MIXED if p[0] % 16) == [999, 1000]
    assert any(p[2] % 64 == 56 and p[2] > 64 for p in ALIGNED) and (4096, 64, 5) in ALIGNED
    assert pack([(GATE, 1, GATE)]) == [[(0, 0, 0)]]          # the gate has slot 0 to itself
    for parts in (ALIGNED, MIXED):
        slots = pack(parts)
        assert [[k for k, _, _ in s] for s in slots] == CLAIMED + [[9]]
        assert all(sum(parts[k][1] for k, _, _ in s) == LANES for s in slots[:7])
        assert [lane0 for _, _, lane0 in slots[1]] == [0, 40]
        assert [off for _, off, _ in slots[1]] == [0, (part_bytes(parts[1]) + 255) & ~255]
        # the gate runs in slot 0, so these are slots 1 .. 7 of 8: the last part finds none free
        assert 1 + len(CLAIMED) == SLOTS
        arena = [(1 + i) * SLOT + off for i, s in enumerate(slots[:7]) for _, off, _ in s]
        assert min(arena) >= GiB and sum(1 for a in arena if a >= 5 * GiB) >= 3
        assert sum(1 for a in arena if a >= B32) >= 4 and max(arena) < 8 * GiB
        # one piece of each part: a 64-lane slot needs only a few MiB of its GiB
        assert max(part_bytes(p) for p in parts) < 8 << 20
    small = [(1 << 18, 3, 1 << 18), (1 << 18, 2, 5)]           # 768 KiB + 256 KiB + 5 > 1 MiB
    assert [[k for k, _, _ in s] for s in pack(small, 1 << 20, 64)] == [[0], [1]]


# --------------------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def gv():
    from downloader_amd.ops import gpu_available, gpuhash
    if not gpu_available():
        pytest.fail("HIP device not visible: the GPU test tier must run on a MI355X")
    assert "gfx950" in gpuhash().arch()
    return gpuhash().GpuVerifier(0, 8 << 20, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", [pytest.param(n, id=f"{n}-seed{HIGH[n][0]}") for n in HIGH])
def test_lane_kernels_at_high_offsets(gv, name, kernel):
    data, offs, lens, want, base = high_table(name)
    got = gv.hash_lanes(data, list(offs), list(lens), kernel, base=base)
    assert len(got) == 20 * len(offs)
    bad = [i for i in range(len(offs)) if got[20 * i:20 * i + 20] != want[i]]
    if bad:
        i = bad[0]
        pytest.fail(f"{kernel} on {name} at base {base}: {len(bad)} of {len(offs)} lanes wrong, "
                    f"first lane {i} (off, len) = ({base} + {offs[i]}, {lens[i]}): got "
                    f"{got[20 * i:20 * i + 20].hex()}, hashlib {want[i].hex()}")


@pytest.mark.gpu
def test_hash_lanes_refuses_bad_bases(gv):
    data = random.Random(510).randbytes(4096)
    want = hashlib.sha1(data[16:116]).digest()
    for kernel in KERNELS:
        for base in (8, -256, 8 * GiB + 256, 1 << 40):
            with pytest.raises(ValueError):
                gv.hash_lanes(data, [16], [100], kernel, base=base)
        assert gv.hash_lanes(data, [16], [100], kernel, base=256) == want
    assert gv.hash_lanes(data, [16], [100], "split", 0) == want
    assert gv.hash_lanes(data, [4000], [96], "lanes16", base=8 * GiB) == \
        hashlib.sha1(data[4000:]).digest()                   # the largest base, up to the pad


def _until(what, cond, errors):
    """Poll `cond` (a few hundred microseconds a turn); a failed part or 20 s end the test."""
    end = time.perf_counter() + 20
    while not cond():
        if errors:
            pytest.fail(f"{what}: {errors[0]!r}")
        if time.perf_counter() > end:
            pytest.fail(f"{what}: not reached in 20 s")
        time.sleep(0.0002)


RUNS = [
    pytest.param(ALIGNED, "split", "sha1_lanes_split", 600, id="aligned-split-seed600"),
    pytest.param(ALIGNED, "lanes", "sha1_lanes", 620, id="aligned-lanes16-seed620"),
    pytest.param(MIXED, "split", "sha1_lanes_split", 640, id="mixed-lanes1-seed640"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("parts,env,kernel,seed", RUNS)
def test_part_hasher_launch_over_many_gib_slots(monkeypatch, parts, env, kernel, seed):
    """Production geometry (8 slots of 1 GiB in one arena), 64 lanes a slot so slots fill with
    little data. A 16 MiB one-piece part holds the only compute stream while ten parts arrive in
    a fixed order and fill slots 1 .. 7 as test_follower_parts_fill_the_slots_they_claim lays
    out; the launch after the gate carries all seven - arena offsets of 1 .. 8 GiB - and the
    tenth part waits for a slot. With `MIXED` two parts are off 16 bytes, so that whole launch
    runs on sha1_lanes<1>."""
    from downloader_amd.ops import gpu_available, gpuhash
    if not gpu_available():
        pytest.fail("HIP device not visible: the GPU test tier must run on a MI355X")
    monkeypatch.setenv("STAGER_SHA1_KERNEL", env)
    h = gpuhash().PartHasher(0, SLOT, SLOTS, 1, LANES)
    before = h.stats()
    assert before["kernel"] == kernel and before["compute_streams"] == 1
    gate = random.Random(seed).randbytes(GATE)
    datas = [random.Random(seed + 1 + k).randbytes(part_bytes(p)) for k, p in enumerate(parts)]
    got, done_at, errors = {}, {}, []

    def submit(key, data, piece):
        try:
            got[key] = h.hash(data, piece)
            done_at[key] = time.perf_counter()
        except Exception as e:               # reported by the polling loop / after the join
            errors.append((key, e))

    threads = [threading.Thread(target=submit, args=("gate", gate, GATE))]
    threads[0].start()
    _until("the gate's launch", lambda: h.stats()["launches"] == before["launches"] + 1, errors)
    t0 = time.perf_counter()
    for k, (part, data) in enumerate(zip(parts, datas)):
        threads.append(threading.Thread(target=submit, args=(k, data, part[0])))
        threads[-1].start()
        # in this order: which parts share a slot depends on it
        _until(f"part {k} queued",
               lambda: h.stats()["submitted"] >= before["submitted"] + 2 + k, errors)
    t_queued = time.perf_counter()
    for t in threads:
        t.join()
    assert not errors, errors
    st = h.stats()
    print(f"{kernel} seed {seed}: followers queued in {(t_queued - t0) * 1e3:.2f} ms, the gate's "
          f"launch ran {(done_at['gate'] - t0) * 1e3:.1f} ms from its start being seen; "
          f"launches {st['launches']}, multi-slot {st['multi_slot_launches']}, "
          f"most slots in one {st['max_launch_slots']}, most lanes {st['max_batch_lanes']}")
    assert st["multi_slot_launches"] - before["multi_slot_launches"] >= 1, st
    assert st["max_launch_slots"] >= 6, st
    assert not st["broken"] and st["pending"] == 0, st
    assert got["gate"] == hashlib.sha1(gate).digest()
    for k, (part, data) in enumerate(zip(parts, datas)):
        want = ref(data, part[0])
        assert len(got[k]) == len(want) == 20 * part[1]
        bad = [i for i in range(part[1]) if got[k][20 * i:20 * i + 20] != want[20 * i:20 * i + 20]]
        assert not bad, (f"part {k} {part} (seed {seed + 1 + k}): {len(bad)} pieces wrong, "
                         f"first {bad[0]}")
    del h


@pytest.mark.gpu
def test_part_hasher_refuses_parts_that_fit_no_slot():
    from downloader_amd.ops import gpu_available, gpuhash
    if not gpu_available():
        pytest.fail("HIP device not visible: the GPU test tier must run on a MI355X")
    h = gpuhash().PartHasher(0, 1 << 20, 2, 1, 64)
    rng = random.Random(660)
    good = rng.randbytes(63 * 1008 + 56)
    refused = [
        (rng.randbytes(65 * 64), 64),                    # 65 pieces, 64 lanes a slot
        (rng.randbytes(64 * 64 + 1), 64),                # the 65th is one byte
        (rng.randbytes((1 << 20) + 16), 1 << 19),        # 3 pieces, 16 bytes over the slot
        (rng.randbytes((1 << 20) + 1), 1 << 21),         # one piece, one byte over
        (b"", 64),
        (bytearray(), 16384),
    ]
    for data, piece in refused:
        with pytest.raises(RuntimeError):
            h.hash(data, piece)
        st = h.stats()
        assert not st["broken"] and st["pending"] == 0, (len(data), piece, st)
        assert h.hash(good, 1008) == ref(good, 1008), (len(data), piece)
    full = rng.randbytes(1 << 20)                        # exactly a slot, exactly 64 lanes
    assert h.hash(full, 1 << 14) == ref(full, 1 << 14)
    assert h.stats()["submitted"] == len(refused) + 1
    del h


# ------------------------------------------- 3. streamed verify: chunk above the staging slot
S_PIECE = 262144 + 60
S_TOTAL = 5 * S_PIECE + 63


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,seed", [
    pytest.param(1 << 20, 701, id="chunk-1MiB-seed701"),
    pytest.param(S_PIECE, 702, id="chunk-is-the-piece-seed702"),
    pytest.param(65536 + 64, 703, id="chunk-one-block-over-the-slot-seed703"),
])
def test_streamed_chunk_larger_than_the_staging_slot(tmp_path, chunk, seed):
    """A 64 KiB staging slot and a chunk above it: the chunk is clamped to the slot (it was read
    and copied whole, one lane a window, into slots a fraction of its size)."""
    from downloader_amd.ops import gpu_available, gpuhash
    if not gpu_available():
        pytest.fail("HIP device not visible: the GPU test tier must run on a MI355X")
    g = gpuhash().GpuVerifier(0, 65536, 2)
    data = bytearray(random.Random(seed).randbytes(S_TOTAL))
    hashes = ref(bytes(data), S_PIECE)
    p = tmp_path / "s"
    p.write_bytes(bytes(data))
    files = [(str(p), S_TOTAL)]
    which = [5, 2, 0, 3]
    assert g.verify_files_streamed(files, S_PIECE, hashes, chunk)[0] == b"\x01" * 6
    assert g.verify_files_streamed(files, S_PIECE, hashes, chunk, which=which)[0] == b"\x01" * 4
    assert g.batch_bytes == 65536
    data[_flip_offset(S_PIECE, 2)] ^= 0x08
    p.write_bytes(bytes(data))
    assert list(g.verify_files_streamed(files, S_PIECE, hashes, chunk)[0]) == [1, 1, 0, 1, 1, 1]
    ok, _ = g.verify_files_streamed(files, S_PIECE, hashes, chunk, which=which)
    assert list(ok) == [1, 0, 1, 1]


@pytest.mark.gpu
def test_streamed_slot_under_one_block_is_grown(tmp_path):
    """A staging slot that cannot hold one 64-byte block (as after a failed grow) is grown to the
    chunk before anything is read into it."""
    from downloader_amd.ops import gpu_available, gpuhash
    if not gpu_available():
        pytest.fail("HIP device not visible: the GPU test tier must run on a MI355X")
    g = gpuhash().GpuVerifier(0, 32, 2)
    data = random.Random(704).randbytes(9 * 1000 + 57)
    hashes = ref(data, 1000)
    p = tmp_path / "t"
    p.write_bytes(data)
    assert g.verify_files_streamed([(str(p), len(data))], 1000, hashes, 4096)[0] == b"\x01" * 10
    assert g.batch_bytes == 960                              # min(chunk, piece) in whole blocks
    assert g.hash_buffer(data, 1000) == hashes


B_SIZES = [70_001, 33_333, 50_000]


@functools.lru_cache(maxsize=None)
def broken_blob():
    return tuple(random.Random(710 + i).randbytes(n) for i, n in enumerate(B_SIZES))


def touching(piece, lo, hi, total):
    """Pieces with a byte in [lo, hi)."""
    return [i for i in range((total + piece - 1) // piece)
            if i * piece < hi and min((i + 1) * piece, total) > lo]


@pytest.mark.gpu
@pytest.mark.parametrize("piece", [1000, 16384])
@pytest.mark.parametrize("case", ["missing-middle-file", "short-last-file"])
def test_gpu_verify_paths_on_broken_storage(gv, tmp_path, case, piece):
    """Seeds 710 - 712 (one per file). A piece with a byte that cannot be read is 0, every other
    piece keeps its own verdict - on the batched and the streamed path, and through `which`."""
    blobs = broken_blob()
    total = sum(B_SIZES)
    hashes = ref(b"".join(blobs), piece)
    n = len(hashes) // 20
    files = []
    for i, d in enumerate(blobs):
        (tmp_path / f"f{i}").write_bytes(d)
        files.append((str(tmp_path / f"f{i}"), len(d)))
    assert gv.verify_files(files, piece, hashes) == b"\x01" * n
    assert gv.verify_files_streamed(files, piece, hashes)[0] == b"\x01" * n
    if case == "missing-middle-file":
        os.unlink(files[1][0])
        lost = touching(piece, B_SIZES[0], B_SIZES[0] + B_SIZES[1], total)
        assert len(lost) == (34 if piece == 1000 else 3)
    else:
        os.truncate(files[2][0], B_SIZES[2] - 10)
        lost = touching(piece, total - 10, total, total)
        assert lost == [n - 1]
    want = bytes(0 if i in lost else 1 for i in range(n))
    assert 0 < len(lost) < n
    assert gv.verify_files(files, piece, hashes) == want
    assert gv.verify_files_streamed(files, piece, hashes)[0] == want
    which = [n - 1, lost[0], 0, lost[-1], 1]              # unsorted: lost, good and the last piece
    ok, _ = gv.verify_files_streamed(files, piece, hashes, which=which)
    assert ok == bytes(want[i] for i in which) and 0 in ok and 1 in ok


# --------------------------------------------- 4. the sha1_pieces arms of the kernel benches
VARIANTS = ["default", "plain", "noprefetch"]
V_PIECES = [64, 128, 192, 1008, 16384]                    # 1, 2, 3, 15 and 256 blocks
V_LAST = [55, 56, 63]


@functools.lru_cache(maxsize=None)
def variant_data(piece, last):
    seed = 800 + V_PIECES.index(piece) * 3 + V_LAST.index(last)
    data = random.Random(seed).randbytes(130 * piece + last)
    return seed, data, ref(data, piece)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("piece,last", [
    pytest.param(p, V_LAST[(i + j) % 3],
                 id=f"piece{p}-last{V_LAST[(i + j) % 3]}-seed{800 + i * 3 + (i + j) % 3}")
    for i, p in enumerate(V_PIECES) for j in range(2)])
def test_bench_only_piece_kernels_match_hashlib(gv, variant, piece, last):
    seed, data, want = variant_data(piece, last)
    got = gv.hash_pieces_variant(data, piece, variant)
    assert len(got) == len(want) == 131 * 20
    bad = [i for i in range(131) if got[20 * i:20 * i + 20] != want[20 * i:20 * i + 20]]
    assert not bad, (f"{variant}, piece {piece}, last {last} (seed {seed}): {len(bad)} pieces "
                     f"wrong, first {bad[0]}")


@pytest.mark.gpu
def test_hash_pieces_variant_refusals(gv):
    data = random.Random(830).randbytes(5 * 1024 + 9)
    for variant in VARIANTS:
        assert gv.hash_pieces_variant(data, 1024, variant) == ref(data, 1024)
        for piece in (1000, 1028, 8, 0, -16):
            with pytest.raises(ValueError):
                gv.hash_pieces_variant(data, piece, variant)
        with pytest.raises(ValueError):
            gv.hash_pieces_variant(b"", 1024, variant)
    for variant in ("", "prefetch", "Default"):
        with pytest.raises(ValueError):
            gv.hash_pieces_variant(data, 1024, variant)
    assert gv.hash_pieces_variant(data[:40], 1024, "plain") == hashlib.sha1(data[:40]).digest()
