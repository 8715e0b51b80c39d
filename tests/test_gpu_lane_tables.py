"""The PartHasher kernels (sha1_lanes_split, sha1_lanes<16>, sha1_lanes<1>), the streamed
sha1_chunk kernel and GpuVerifier's host paths against hashlib on exact, seeded inputs.

``GpuVerifier.hash_lanes`` launches one kernel on a lane table given here, so every tail
remainder, lanes that end at very different blocks, partial workgroups and a tail read that
runs into the arena pad meet a reference - through ``PartHasher.hash`` every lane of a part has
one length and which parts share a launch depends on timing. Every comparison is bit-exact.
"""
from __future__ import annotations

import functools
import hashlib
import random

import pytest

KERNELS = ["split", "split_idle", "lanes16", "lanes1"]
LONG = 65536 + 57                   # 1,026 blocks (1,024 whole + 57 bytes: two padding blocks)
PARTIAL_N = [1, 16, 63, 65, 130]


def blocks(length):
    """64-byte blocks SHA-1 runs for a message: whole blocks + one or two padding blocks."""
    return (length >> 6) + (2 if (length & 63) >= 56 else 1)


def align16(x):
    return (x + 15) & ~15


# ------------------------------------------------------------------ lane tables (no device)
def tails_table(stride=256, shift=0):
    """192 lanes, lane i = i bytes: every remainder 0..63 at 0, 1 and 2 whole blocks."""
    offs = [stride * i + shift for i in range(192)]
    lens = list(range(192))
    return offs, lens, offs[-1] + 256


def ragged_lengths(n):
    """Lane 63 is 1,026 blocks long, every other lane j (j * 997) % 5000 bytes (1..79 blocks)."""
    return [LONG if j == 63 else (j * 997) % 5000 for j in range(n)]


def packed(lens, slack=0):
    """Lanes one after another, each start rounded up to 16 bytes."""
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at = align16(at + n)
    return offs, list(lens), offs[-1] + lens[-1] + slack


def ragged_table(long_first=False):
    lens = ragged_lengths(64)
    if long_first:
        lens = [lens[63]] + lens[:63]
    return packed(lens, slack=100)


def partial_table(n):
    return packed(ragged_lengths(n), slack=100)


def edge_table(rem):
    """The last lane ends exactly at len(data): its 64-byte raw tail read runs into the pad."""
    lens = [100, 64, 1000, 0, 55, 4096 + rem]
    offs, lens, size = packed(lens)
    assert size == offs[-1] + lens[-1]
    if rem == 0:                    # and an empty lane that starts at the very end
        offs.insert(3, size)
        lens.insert(3, 0)
    return offs, lens, size


def shared_table():
    """Descending addresses, and lanes that start at one offset with different lengths."""
    offs, lens, size = packed(ragged_lengths(70)[:63] + [64 * 9 + 56, 120, 7, 4096, 63, 1, 0],
                              slack=64)
    offs, lens = offs[::-1], lens[::-1]
    # lanes 10 / 20 / 30 again with other lengths (inside the data: shorter, or up to the end)
    for i, n in ((10, 55), (20, lens[20] + 16), (30, 0)):
        offs.append(offs[i])
        lens.append(min(n, size - offs[i]))
    return offs, lens, size


TABLES = {
    "tails": (101, tails_table),
    "ragged-long-last": (102, ragged_table),
    "ragged-long-first": (103, functools.partial(ragged_table, True)),
    **{f"partial-n{n}": (110 + k, functools.partial(partial_table, n))
       for k, n in enumerate(PARTIAL_N)},
    "edge-rem0": (120, functools.partial(edge_table, 0)),
    "edge-rem63": (121, functools.partial(edge_table, 63)),
    "shared-unordered": (130, shared_table),
}
UNALIGNED = ("tails-unaligned", 140, functools.partial(tails_table, 257, 1))


@functools.lru_cache(maxsize=None)
def table(name):
    """(data, offsets, lengths, hashlib digests) of a table: built once, immutable."""
    seed, build = TABLES[name] if name in TABLES else UNALIGNED[1:]
    offs, lens, size = build()
    data = random.Random(seed).randbytes(size)
    want = tuple(hashlib.sha1(data[o:o + n]).digest() for o, n in zip(offs, lens))
    return data, tuple(offs), tuple(lens), want


def check_lanes(gv, name, kernel):
    data, offs, lens, want = table(name)
    got = gv.hash_lanes(data, list(offs), list(lens), kernel)
    assert len(got) == 20 * len(offs)
    bad = [i for i in range(len(offs)) if got[20 * i:20 * i + 20] != want[i]]
    if bad:
        i = bad[0]
        pytest.fail(f"{kernel} on {name}: {len(bad)} of {len(offs)} lanes wrong, first lane {i} "
                    f"(off, len) = ({offs[i]}, {lens[i]}): got {got[20 * i:20 * i + 20].hex()}, "
                    f"hashlib {want[i].hex()}")


def test_lane_tables_cover_what_they_claim():
    offs, lens, size = tails_table()
    assert len(lens) == 192 and lens[0] == 0
    assert {(n >> 6, n & 63) for n in lens} == {(b, r) for b in (0, 1, 2) for r in range(64)}
    assert all(o % 16 == 0 for o in offs) and all(o + n <= size for o, n in zip(offs, lens))
    longest = [max(blocks(n) for n in lens[g:g + 64]) for g in range(0, 192, 64)]
    assert longest == [2, 3, 4]                   # the split kernel's M: both parities
    assert any(m % 2 for m in longest) and any(m % 2 == 0 for m in longest)
    uoffs, ulens, usize = UNALIGNED[2]()
    assert ulens == lens and all(o % 16 for o in uoffs[:3]) and uoffs[-1] + ulens[-1] <= usize
    assert {o % 16 for o in uoffs} == set(range(16))
    for first in (False, True):
        _, rl, _ = ragged_table(first)
        assert len(rl) == 64 and rl.index(LONG) == (0 if first else 63)
        others = [blocks(n) for n in rl if n != LONG]
        assert blocks(LONG) == 1026 and min(others) == 1 and max(others) == 79
    assert [len(partial_table(n)[0]) for n in PARTIAL_N] == [1, 16, 63, 65, 130]
    assert partial_table(65)[1][:64] == ragged_table()[1]
    for rem in (0, 63):
        eo, el, esize = edge_table(rem)
        assert eo[-1] + el[-1] == esize and el[-1] & 63 == rem
    so, sl, ssize = shared_table()
    assert so[:70] == sorted(so[:70], reverse=True)
    assert any(so.count(o) > 1 and len({n for p, n in zip(so, sl) if p == o}) > 1 for o in so)
    for name in list(TABLES) + [UNALIGNED[0]]:
        data, o, n, want = table(name)
        assert len(o) == len(n) == len(want) >= 1 and len(data) <= 512 << 10
        assert all(0 <= a and 0 <= b and a + b <= len(data) for a, b in zip(o, n))
        if name in TABLES:
            assert all(a % 16 == 0 for a in o)


# --------------------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def gv():
    from downloader_amd.ops import gpu_available, gpuhash
    if not gpu_available():
        pytest.fail("HIP device not visible: the GPU test tier must run on a MI355X")
    assert "gfx950" in gpuhash().arch()
    return gpuhash().GpuVerifier(0, 8 << 20, 4)


def ref(data, piece):
    return b"".join(hashlib.sha1(data[i:i + piece]).digest() for i in range(0, len(data), piece))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", [pytest.param(n, id=f"{n}-seed{TABLES[n][0]}") for n in TABLES])
def test_lane_kernels_match_hashlib(gv, name, kernel):
    check_lanes(gv, name, kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [pytest.param(UNALIGNED[0], id=f"{UNALIGNED[0]}-seed{UNALIGNED[1]}")])
def test_byte_load_kernel_on_unaligned_lanes(gv, name):
    check_lanes(gv, name, "lanes1")


@pytest.mark.gpu
def test_hash_lanes_refuses_bad_tables(gv):
    data = random.Random(150).randbytes(4096)
    assert gv.hash_lanes(data, [16], [100], "split") == hashlib.sha1(data[16:116]).digest()
    for kernel in ("split", "split_idle", "lanes16"):
        with pytest.raises(ValueError):
            gv.hash_lanes(data, [0, 8], [64, 64], kernel)          # lane 1 off 16 bytes
    assert gv.hash_lanes(data, [8], [64], "lanes1") == hashlib.sha1(data[8:72]).digest()
    for kernel in KERNELS:
        with pytest.raises(ValueError):
            gv.hash_lanes(data, [0, 4000], [64, 97], kernel)       # one byte past the end
        with pytest.raises(ValueError):
            gv.hash_lanes(data, [4112], [0], kernel)               # starts past the end
        with pytest.raises(ValueError):
            gv.hash_lanes(data, [], [], kernel)                    # empty table
        with pytest.raises(ValueError):
            gv.hash_lanes(data, [0, 64], [64], kernel)             # a length is missing
        with pytest.raises(ValueError):
            gv.hash_lanes(data, [-16], [64], kernel)
        with pytest.raises(ValueError):
            gv.hash_lanes(data, [0], [-1], kernel)
    with pytest.raises(ValueError):
        gv.hash_lanes(data, [0], [64], "lanes4")                   # unknown kernel
    assert gv.hash_lanes(data, [4000], [96], "lanes16") == hashlib.sha1(data[4000:]).digest()


# ------------------------------------------------------------ sha1_chunk (streamed verify)
def _flip_offset(piece, p):
    """A byte inside the final partial block of piece p."""
    assert piece & 63
    return p * piece + (piece & ~63) + (piece & 63) // 2


STREAMED = [
    # piece, chunk (None: the default), total, seed
    pytest.param(65596, 65536, 5 * 65596 + 63, 201, id="second-chunk-60B-two-pad-blocks-seed201"),
    pytest.param(4096 + 55, 4096, 40 * (4096 + 55), 202, id="last-chunk-55B-seed202"),
    pytest.param(4096 + 56, 4096, 40 * (4096 + 56), 203, id="last-chunk-56B-seed203"),
    pytest.param(48, None, 48 * 130 + 7, 204, id="piece-48-chunk-clamped-to-64-seed204"),
    pytest.param(1000, None, 1000 * 70 + 333, 205, id="piece-1000-chunk-960-seed205"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("piece,chunk,total,seed", STREAMED)
def test_streamed_chunk_edges(gv, tmp_path, piece, chunk, total, seed):
    data = bytearray(random.Random(seed).randbytes(total))
    hashes = ref(bytes(data), piece)
    n = len(hashes) // 20
    p = tmp_path / "s"
    p.write_bytes(bytes(data))
    files = [(str(p), total)]
    args = (files, piece, hashes) + (() if chunk is None else (chunk,))
    ok, _ = gv.verify_files_streamed(*args)
    assert ok == b"\x01" * n
    bad = n // 2
    data[_flip_offset(piece, bad)] ^= 0x10
    p.write_bytes(bytes(data))
    ok, _ = gv.verify_files_streamed(*args)
    assert [i for i, v in enumerate(ok) if not v] == [bad]


@pytest.mark.gpu
def test_streamed_chunk_edges_two_windows(tmp_path):
    """3 lanes per window, 6 pieces: the 63-byte last piece finishes in the first window's first
    round, its neighbours take a 60-byte second chunk (two padding blocks, no whole block)."""
    from downloader_amd.ops import gpuhash
    piece, chunk, total = 65596, 65536, 5 * 65596 + 63
    g = gpuhash().GpuVerifier(0, 3 * chunk, 4)
    data = bytearray(random.Random(206).randbytes(total))
    hashes = ref(bytes(data), piece)
    p = tmp_path / "w"
    p.write_bytes(bytes(data))
    files = [(str(p), total)]
    which = [5, 0, 3, 1, 4, 2]
    assert g.verify_files_streamed(files, piece, hashes, chunk)[0] == b"\x01" * 6
    assert g.verify_files_streamed(files, piece, hashes, chunk, which=which)[0] == b"\x01" * 6
    data[_flip_offset(piece, 3)] ^= 0x02
    p.write_bytes(bytes(data))
    ok, _ = g.verify_files_streamed(files, piece, hashes, chunk, which=which)
    assert list(ok) == [1, 1, 0, 1, 1, 1]
    ok, _ = g.verify_files_streamed(files, piece, hashes, chunk)
    assert list(ok) == [1, 1, 1, 0, 1, 1]


# ------------------------------------------------------------------- GpuVerifier host paths
@pytest.mark.gpu
def test_hash_buffer_grows_its_staging_slots():
    """A piece larger than the staging slot: grow() reallocates both slots; they then serve
    several batches of small pieces."""
    from downloader_amd.ops import gpuhash
    g = gpuhash().GpuVerifier(0, 1 << 20, 2)
    assert g.batch_bytes == 1 << 20
    piece = (1 << 20) + 4096
    data = random.Random(301).randbytes(3 * piece + 777)
    assert g.hash_buffer(data, piece) == ref(data, piece)
    assert g.batch_bytes >= piece
    data = random.Random(302).randbytes(200 * 16384 + 5)       # 64 pieces a batch: 4 batches
    assert g.hash_buffer(data, 16384) == ref(data, 16384)


@pytest.mark.gpu
def test_reported_hip_error_does_not_come_back_from_the_next_launch(gv):
    """A HIP error that was raised once (here: a PartHasher whose arena cannot fit in HBM)
    stayed behind as the thread's last error, and the thread's next launch - checked with
    hipGetLastError() - failed with "out of memory" although nothing was wrong with it."""
    from downloader_amd.ops import gpuhash
    _, total = gpuhash().mem_info(0)
    slot = 32 << 30
    with pytest.raises(RuntimeError):
        gpuhash().PartHasher(0, slot, int(total // slot) + 2, 1, 64)
    data = random.Random(320).randbytes(70 * 1024 + 9)
    assert gv.hash_buffer(data, 1024) == ref(data, 1024)
    assert gv.hash_lanes(data, [0, 64], [119, 1000], "split") == \
        hashlib.sha1(data[:119]).digest() + hashlib.sha1(data[64:1064]).digest()


@pytest.mark.gpu
@pytest.mark.parametrize("piece,seed", [pytest.param(1000, 311, id="piece1000-dword-seed311"),
                                        pytest.param(999, 312, id="piece999-byte-seed312")])
def test_verify_files_compare_path_small_pieces(gv, tmp_path, piece, seed):
    """The kernels' own digest compare (`expected`) on the dword- and byte-load paths."""
    rng = random.Random(seed)
    sizes = [70_001, 33_333]
    files, blob = [], b""
    for i, n in enumerate(sizes):
        d = rng.randbytes(n)
        (tmp_path / f"f{i}").write_bytes(d)
        files.append((str(tmp_path / f"f{i}"), n))
        blob += d
    hashes = ref(blob, piece)
    n = len(hashes) // 20
    assert gv.verify_files(files, piece, hashes) == b"\x01" * n
    at = 12_345                                   # in the second file
    b = bytearray(blob[sizes[0]:])
    b[at] ^= 0x80
    (tmp_path / "f1").write_bytes(bytes(b))
    ok = gv.verify_files(files, piece, hashes)
    assert [i for i, v in enumerate(ok) if not v] == [(sizes[0] + at) // piece]


@pytest.mark.gpu
@pytest.mark.parametrize("piece", [1, 55, 56, 63, 65, 119, 120, 184])
def test_hash_buffer_every_lane_on_a_padding_boundary(gv, piece):
    """Whole pieces only (130 of them, three workgroups): every lane, not just the last, sits
    at the 55 / 56 padding boundary or a byte off a block; 56, 120 and 184 take the dword
    loads, the others the byte loads."""
    data = random.Random(400 + piece).randbytes(130 * piece)
    got, want = gv.hash_buffer(data, piece), ref(data, piece)
    bad = [i for i in range(130) if got[20 * i:20 * i + 20] != want[20 * i:20 * i + 20]]
    assert not bad, f"piece {piece} (seed {400 + piece}): first wrong piece {bad[0]} of {len(bad)}"
