"""The verdicts of the device: one byte per piece, 1 = "keep these bytes".

In production the gfx950 SHA-1 kernels do not return digests: ``sha1_pieces`` (its ``expected``
branch) and ``sha1_chunk`` compare on the device, each with its own indexing, and ``run_batches``
/ ``verify_files_streamed`` carry the expected digests in and the verdict bytes out. A wrong 0
costs a refetch, a wrong 1 stages corrupt data. The tables here hold that side to ``hashlib``
and to the host's ``verify_pieces``, bit-exact:

* near misses: an expected digest one bit off the true one, every bit 0..159 once;
* ``verify_files`` over many batches (``expected + first * 20``, both meta slots, a partial last
  batch, ``ensure_meta`` and ``grow()`` on the compare path);
* stale state: good -> all bad -> good on one verifier, and a file that disappears after a good
  call, when the staging slot still holds the good bytes;
* a seeded differential with data and hash list both tampered with, and ``which`` unsorted and
  with duplicates.

The tables are built without a device, and ``test_verdict_tables_cover_what_they_claim`` runs
their reference side (``verdicts()`` against the host ``verify_pieces``) on any machine.
"""
from __future__ import annotations

import functools
import hashlib
import os
import random

import pytest


# ------------------------------------------------------------------------ helpers (no device)
def digests(data, piece):
    return b"".join(hashlib.sha1(data[i:i + piece]).digest() for i in range(0, len(data), piece))


def verdicts(data, piece, hashes):
    """The hashlib verdict list: 1 where piece k of ``data`` has the digest ``hashes`` lists."""
    assert len(hashes) == 20 * ((len(data) + piece - 1) // piece)
    return [int(hashlib.sha1(data[i:i + piece]).digest() == hashes[20 * k:20 * k + 20])
            for k, i in enumerate(range(0, len(data), piece))]


def storage(sizes, seed):
    """One seeded blob per file."""
    rng = random.Random(seed)
    return tuple(rng.randbytes(n) for n in sizes)


def write_storage(where, data, sizes):
    """``data`` cut into files of ``sizes`` under ``where``: the (path, length) list."""
    assert len(data) == sum(sizes)
    files, at = [], 0
    for i, n in enumerate(sizes):
        p = os.path.join(str(where), f"f{i}")
        with open(p, "wb") as f:
            f.write(data[at:at + n])
        files.append((p, n))
        at += n
    return files


def flip_digest_bit(hashes, j, bit):
    """Bit ``bit`` (0 = the top bit of byte 0 .. 159) of piece j's expected digest."""
    assert 0 <= bit < 160
    hashes[20 * j + bit // 8] ^= 0x80 >> (bit % 8)


def flip_data_byte(data, piece, j, at=-1, mask=0x01):
    """Byte ``at`` of piece j (default: its last byte)."""
    start, end = j * piece, min((j + 1) * piece, len(data))
    pos = end - 1 if at < 0 else start + at
    assert start <= pos < end and mask
    data[pos] ^= mask


def host_verdicts(files, piece, hashes, which=()):
    from downloader_amd.ops import native
    return list(native().verify_pieces(files, piece, hashes, list(which), 0))


def same(got, want, what):
    got, want = list(got), list(want)
    assert len(got) == len(want), f"{what}: {len(got)} verdicts for {len(want)} pieces"
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    if bad:
        i = bad[0]
        pytest.fail(f"{what}: {len(bad)} of {len(want)} verdicts wrong, first at {i}: device "
                    f"{got[i]}, reference {want[i]} (all: {bad[:20]})")


# ------------------------------------------------------------------- a. the near-miss table
NEAR_SEEDS = {1024: 501, 1000: 502, 999: 503}     # sha1_pieces<16>, <4>, <1>
NEAR_N = 163
NEAR_WANT = bytes([0] * 160 + [1, 0, 1])
NEAR_WHICH_SEED = 510


@functools.lru_cache(maxsize=None)
def near_miss_table(piece):
    """162 whole pieces and a 37-byte last one. Pieces 0..159: bit j of the expected digest
    flipped; 160 untouched; 161 its last data byte flipped; 162 short and untouched.
    -> (good data, good hashes, tampered data, tampered hashes)."""
    good_data = random.Random(NEAR_SEEDS[piece]).randbytes(162 * piece + 37)
    good = digests(good_data, piece)
    data, hashes = bytearray(good_data), bytearray(good)
    for j in range(160):
        flip_digest_bit(hashes, j, j)
    flip_data_byte(data, piece, 161)
    return good_data, good, bytes(data), bytes(hashes)


def near_which():
    return random.Random(NEAR_WHICH_SEED).sample(range(NEAR_N), NEAR_N)


SHORT_SEED = 520
SHORT_PIECE = 1024


@functools.lru_cache(maxsize=None)
def short_last_table(bit):
    """Five whole pieces and a 37-byte one whose expected digest alone is one bit off."""
    data = random.Random(SHORT_SEED + bit).randbytes(5 * SHORT_PIECE + 37)
    good = digests(data, SHORT_PIECE)
    hashes = bytearray(good)
    flip_digest_bit(hashes, 5, bit)
    return data, good, bytes(hashes)


# ------------------------------------------------------ b. many batches on the compare path
BATCH_SLOT = 64 * 1024
NEAR_BITS = [0, 159, 31, 32, 127, 96]


def batch_edges(n, per):
    """(pieces with flipped data, near-miss pieces): the first and the last piece of every
    batch of ``per`` and the last piece of all; piece first + 1 of every batch."""
    firsts = list(range(0, n, per))
    bad = {f for f in firsts} | {min(f + per, n) - 1 for f in firsts} | {n - 1}
    near = [f + 1 for f in firsts]
    return bad, near


@functools.lru_cache(maxsize=None)
def batch_table(piece, whole, short, seed):
    """``whole`` pieces and one of ``short`` bytes, tampered with on the edges of the batches a
    64 KiB slot cuts them into. -> (data, hashes, want)."""
    per = BATCH_SLOT // piece
    data = bytearray(random.Random(seed).randbytes(whole * piece + short))
    hashes = bytearray(digests(bytes(data), piece))
    n = whole + 1
    bad, near = batch_edges(n, per)
    for k, j in enumerate(sorted(bad)):
        flip_data_byte(data, piece, j, at=(k * 7) % min(piece, short), mask=0x80 >> (k % 8))
    for k, j in enumerate(near):
        flip_digest_bit(hashes, j, NEAR_BITS[k % len(NEAR_BITS)])
    want = bytes(0 if j in bad or j in near else 1 for j in range(n))
    return bytes(data), bytes(hashes), want


GROW_PIECE = 65536 + 64


@functools.lru_cache(maxsize=None)
def grow_table():
    """Five pieces larger than the slot (the last one short), piece 2 corrupt."""
    data = bytearray(random.Random(533).randbytes(4 * GROW_PIECE + 1000))
    hashes = digests(bytes(data), GROW_PIECE)
    flip_data_byte(data, GROW_PIECE, 2, at=GROW_PIECE - 33, mask=0x04)
    return bytes(data), hashes, bytes([1, 1, 0, 1, 1])


BATCH_STEPS = [
    # name, builder: run in this order on ONE verifier with 64 KiB slots
    ("piece1024-five-batches-seed531", functools.partial(batch_table, 1024, 273, 333, 531)),
    ("piece64-ensure-meta-grows-seed532", functools.partial(batch_table, 64, 2100, 17, 532)),
    ("piece1024-again-seed531", functools.partial(batch_table, 1024, 273, 333, 531)),
    ("piece65600-grow-seed533", grow_table),
]
BATCH_PIECES = [1024, 64, 1024, GROW_PIECE]


# ----------------------------------------------------------------------------- c. stale state
STALE_PIECE = 1000
STALE_ONE = (601, (70_333,))                      # 71 pieces: two batches / two windows
STALE_TWO = (602, (33_333, 20_001))               # 54 pieces: one batch, one window
STALE_SLOT = 64 * 1024


def all_flipped(data, piece, seed):
    rng = random.Random(seed)
    out = bytearray(data)
    for j in range((len(data) + piece - 1) // piece):
        n = min(piece, len(data) - j * piece)
        flip_data_byte(out, piece, j, at=rng.randrange(n), mask=1 << rng.randrange(8))
    return bytes(out)


# ---------------------------------------------------------------- d. the seeded differential
DIFF = {
    "piece4152-chunk1024-slot8k": dict(seed=701, piece=4096 + 56, chunk=1024, slot=8 << 10,
                                       sizes=(5000, 0, 1, 70_000, 3, 33_333)),
    "piece1000-default-chunk-slot64k": dict(seed=702, piece=1000, chunk=None, slot=64 << 10,
                                            sizes=(70_980, 33_333, 95_688)),
    "piece64-chunk64-slot4k": dict(seed=703, piece=64, chunk=64, slot=4 << 10,
                                   sizes=(7000, 12_211)),
    "piece65540-chunk4096-slot64k": dict(seed=704, piece=65536 + 4, chunk=4096, slot=64 << 10,
                                         sizes=(6 * 65540 + 65538, 300_001, 487_715)),
}
FRONT_END = "piece1000-default-chunk-slot64k"


def chunk_and_window(piece, chunk, slot, lanes):
    """verify_files_streamed's chunk and lanes per window for this geometry."""
    ch = max(64, min(65536 if chunk is None else chunk, piece) & ~63)
    ch = min(ch, slot & ~63)
    return ch, max(1, min(lanes, slot // ch))


@functools.lru_cache(maxsize=None)
def diff_table(name):
    """About a tenth of the pieces tampered with in the data, another tenth in the hash list,
    at least one tampered and one clean piece in every streamed window.
    -> (data, hashes, want, which, tampered pieces)."""
    g = DIFF[name]
    piece, rng = g["piece"], random.Random(g["seed"])
    data = bytearray(b"".join(rng.randbytes(n) for n in g["sizes"]))
    hashes = bytearray(digests(bytes(data), piece))
    n = len(hashes) // 20
    _, w = chunk_and_window(piece, g["chunk"], g["slot"], n)
    tenth = max(1, round(n / 10))
    for _ in range(10_000):
        bad_data = set(rng.sample(range(n), tenth))
        bad_hash = set(rng.sample([i for i in range(n) if i not in bad_data], tenth))
        tam = bad_data | bad_hash
        wins = [range(f, min(f + w, n)) for f in range(0, n, w)]
        if all(any(i in tam for i in win) and any(i not in tam for i in win) for win in wins):
            break
    else:
        raise AssertionError(f"{name}: no tampering with every window mixed")
    for j in sorted(bad_data):
        length = min(piece, len(data) - j * piece)
        flip_data_byte(data, piece, j, at=rng.randrange(length), mask=1 << rng.randrange(8))
    for j in sorted(bad_hash):
        flip_digest_bit(hashes, j, rng.randrange(160))
    which = tuple(rng.randrange(n) for _ in range(n + n // 2))
    want = bytes(0 if j in tam else 1 for j in range(n))
    return bytes(data), bytes(hashes), want, which, frozenset(tam)


# ------------------------------------------------------------- e. the tables, without a device
def test_verdict_tables_cover_what_they_claim(tmp_path):
    def on_host(tag, data, sizes, piece, hashes, want, which=()):
        d = tmp_path / tag
        d.mkdir()
        files = write_storage(d, data, sizes)
        assert verdicts(data, piece, hashes) == list(want), tag
        assert host_verdicts(files, piece, hashes) == list(want), tag
        if which:
            assert host_verdicts(files, piece, hashes, which) == [want[i] for i in which], tag

    # a. every digest bit 0..159 flipped exactly once, in a piece of its own
    for piece in NEAR_SEEDS:
        good_data, good, data, hashes = near_miss_table(piece)
        assert len(good) == 20 * NEAR_N and len(data) == 162 * piece + 37
        diff = [good[i] ^ hashes[i] for i in range(len(good))]
        bits = [(i // 20, (i % 20) * 8 + k) for i, x in enumerate(diff) for k in range(8)
                if x & (0x80 >> k)]
        assert bits == [(j, j) for j in range(160)]
        assert [i for i in range(len(data)) if data[i] != good_data[i]] == [162 * piece - 1]
        assert verdicts(good_data, piece, good) == [1] * NEAR_N
        on_host(f"near{piece}", data, (len(data),), piece, hashes, NEAR_WANT, near_which())
    assert sorted(near_which()) == list(range(NEAR_N)) and near_which() != list(range(NEAR_N))
    assert chunk_and_window(1024, 256, 64 * 256, NEAR_N) == (256, 64)    # 64 + 64 + 35 lanes
    for bit in (0, 159):
        data, good, hashes = short_last_table(bit)
        assert [i for i in range(120) if good[i] != hashes[i]] == [100 + bit // 8]
        on_host(f"short{bit}", data, (len(data),), SHORT_PIECE, hashes, [1, 1, 1, 1, 1, 0])

    # b. the tampered pieces sit on the batch edges they claim, for per = 64
    bad, near = batch_edges(274, 64)
    assert sorted(bad) == [0, 63, 64, 127, 128, 191, 192, 255, 256, 273]
    assert near == [1, 65, 129, 193, 257] and not bad & set(near)
    data, hashes, want = batch_table(1024, 273, 333, 531)
    assert len(want) == 274 and [i for i, v in enumerate(want) if not v] == sorted(bad | set(near))
    assert BATCH_SLOT // 1024 == 64 and len(range(0, 274, 64)) == 5 and 274 % 64 == 18
    bad64, near64 = batch_edges(2101, BATCH_SLOT // 64)
    assert sorted(bad64) == [0, 1023, 1024, 2047, 2048, 2100] and near64 == [1, 1025, 2049]
    assert (BATCH_SLOT // 64) * 21 > 64 * 21      # ensure_meta has to grow for piece 64
    assert GROW_PIECE > BATCH_SLOT                # and the slots for the last step
    for (tag, build), piece in zip(BATCH_STEPS, BATCH_PIECES):
        data, hashes, want = build()
        assert 0 in want and 1 in want and len(data) <= 300_000
        on_host(tag, data, (len(data),), piece, hashes, want)

    # d. every streamed window of every differential table holds tampered and clean pieces
    for name, g in DIFF.items():
        data, hashes, want, which, tam = diff_table(name)
        piece, sizes, n = g["piece"], g["sizes"], len(want)
        assert len(data) == sum(sizes) <= 1_300_000
        ch, w = chunk_and_window(piece, g["chunk"], g["slot"], n)
        for f in range(0, n, w):
            win = want[f:f + w]
            assert 0 in win and 1 in win, (name, f)
        assert n > w and len(tam) in (2 * max(1, round(n / 10)),)
        assert len(set(which)) < len(which) and list(which) != sorted(which)
        assert all(0 <= i < n for i in which) and len(which) > w
        # file boundaries inside chunks (not on a chunk edge)
        edges = [sum(sizes[:k]) for k in range(1, len(sizes))]
        assert any((e % piece) % ch for e in edges), name
        on_host(name, data, sizes, piece, hashes, want, which)
    # ... and inside a piece's tail block, where the geometry has one
    for name in ("piece1000-default-chunk-slot64k", "piece65540-chunk4096-slot64k"):
        g = DIFF[name]
        assert g["piece"] & 63 and any(sum(g["sizes"][:k]) % g["piece"] >= g["piece"] & ~63
                                       for k in range(1, len(g["sizes"])))

    # c. which pieces the second file of the two-file storage touches
    first = STALE_TWO[1][0]
    assert first // STALE_PIECE == 33 and first % STALE_PIECE
    assert sum(STALE_TWO[1]) <= STALE_SLOT < sum(STALE_ONE[1])


# --------------------------------------------------------------------------- on the device
def _gpuhash():
    from downloader_amd.ops import gpu_available, gpuhash
    if not gpu_available():
        pytest.fail("HIP device not visible: the GPU test tier must run on a MI355X")
    assert "gfx950" in gpuhash().arch()
    return gpuhash()


@pytest.fixture(scope="module")
def one_batch():
    """256 KiB slots: the 163-piece tables fit ONE batch, so a fault of the compare itself is
    told apart from a fault of the batch plumbing (b and d)."""
    return _gpuhash().GpuVerifier(0, 256 * 1024, 2)


@pytest.fixture(scope="module")
def lanes64():
    """Slots of 64 chunks of 256 bytes: 163 lanes are three windows, the last one partial."""
    return _gpuhash().GpuVerifier(0, 64 * 256, 2)


def run(g, mode, files, piece, hashes, chunk=None, which=None):
    """The verdicts of one device path, as a list."""
    extra = () if chunk is None else (chunk,)
    if mode == "files":
        return list(g.verify_files(files, piece, hashes))
    if mode == "streamed":
        return list(g.verify_files_streamed(files, piece, hashes, *extra)[0])
    assert mode == "which" and which
    return list(g.verify_files_streamed(files, piece, hashes, *extra, which=list(which))[0])


NEAR_ARMS = [
    pytest.param("files", 1024, id="verify_files-piece1024-dwordx4-seed501"),
    pytest.param("files", 1000, id="verify_files-piece1000-dword-seed502"),
    pytest.param("files", 999, id="verify_files-piece999-byte-seed503"),
    pytest.param("streamed", 1024, id="streamed-piece1024-chunk256-seed501"),
    pytest.param("which", 1024, id="streamed-which-permuted-3-windows-seed501-510"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,piece", NEAR_ARMS)
def test_near_miss_digests(one_batch, lanes64, tmp_path, mode, piece):
    """An expected digest one bit off the true one is a 0, whichever of the 160 bits it is."""
    g = lanes64 if mode == "which" else one_batch
    good_data, good, data, hashes = near_miss_table(piece)
    chunk = None if mode == "files" else 256
    which = near_which() if mode == "which" else None
    pick = (lambda v: [v[i] for i in which]) if which else list
    files = write_storage(tmp_path, good_data, (len(good_data),))
    same(run(g, mode, files, piece, good, chunk, which), [1] * NEAR_N, f"{mode} untampered")
    files = write_storage(tmp_path, data, (len(data),))
    got = run(g, mode, files, piece, hashes, chunk, which)
    same(got, pick(NEAR_WANT), f"{mode} piece {piece}: verdict k <-> digest bit k")
    assert got == pick(host_verdicts(files, piece, hashes))


@pytest.mark.gpu
@pytest.mark.parametrize("bit", [pytest.param(0, id="bit0-seed520"),
                                 pytest.param(159, id="bit159-seed679")])
def test_near_miss_on_the_short_last_piece_only(one_batch, lanes64, tmp_path, bit):
    data, good, hashes = short_last_table(bit)
    files = write_storage(tmp_path, data, (len(data),))
    want = [1, 1, 1, 1, 1, 0]
    assert host_verdicts(files, SHORT_PIECE, hashes) == want
    which = [5, 2, 5, 0]
    for g in (one_batch, lanes64):
        for mode in ("files", "streamed", "which"):
            chunk = None if mode == "files" else 256
            ones = run(g, mode, files, SHORT_PIECE, good, chunk, which)
            same(ones, [1] * len(ones), f"{mode} untampered")
            got = run(g, mode, files, SHORT_PIECE, hashes, chunk, which)
            same(got, [want[i] for i in which] if mode == "which" else want, f"{mode} bit {bit}")


@pytest.mark.gpu
def test_near_miss_through_which_with_duplicates(lanes64, tmp_path):
    """Only near-miss pieces, some listed more than once: every lane says 0 (seed 501)."""
    _, good, data, hashes = near_miss_table(1024)
    files = write_storage(tmp_path, data, (len(data),))
    which = [5, 5, 159, 0, 128, 5, 159, 17, 127, 96] * 7          # 70 lanes: two windows
    assert host_verdicts(files, 1024, hashes, which) == [0] * len(which)
    got = run(lanes64, "which", files, 1024, good, 256, which)
    same(got, [1] * len(which), "untampered")
    got = run(lanes64, "which", files, 1024, hashes, 256, which)
    same(got, [0] * len(which), "near misses, duplicates")


@pytest.mark.gpu
def test_verify_files_many_batches_on_the_compare_path(tmp_path):
    """Seeds 531 - 533, one verifier with 64 KiB slots: five batches of 64 pieces with a partial
    last one (`expected + first * 20`, both meta slots, `out_ok + first`), then 1,024 pieces a
    batch (`ensure_meta` grows), the first table again, and pieces larger than the slot
    (`grow()`)."""
    g = _gpuhash().GpuVerifier(0, BATCH_SLOT, 2)
    assert g.batch_bytes == BATCH_SLOT
    for (tag, build), piece in zip(BATCH_STEPS, BATCH_PIECES):
        data, hashes, want = build()
        d = tmp_path / tag
        d.mkdir()
        files = write_storage(d, data, (len(data),))
        assert verdicts(data, piece, hashes) == list(want)
        got = run(g, "files", files, piece, hashes)
        same(got, want, tag)
        assert got == host_verdicts(files, piece, hashes), tag
    assert g.batch_bytes >= GROW_PIECE


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [pytest.param(m, id=f"{m}-seed601-605")
                                  for m in ("files", "streamed", "which")])
def test_no_stale_verdicts_or_bytes(tmp_path, mode):
    """Seeds 601 - 605, one verifier throughout: good -> every piece bad -> good, then a file
    that disappears after a good call with the same geometry - the staging slot still holds its
    good bytes."""
    g = _gpuhash().GpuVerifier(0, STALE_SLOT, 2)
    piece = STALE_PIECE
    seed, sizes = STALE_ONE
    data = b"".join(storage(sizes, seed))
    hashes = digests(data, piece)
    n = len(hashes) // 20
    which = random.Random(603).sample(range(n), n) if mode == "which" else None
    for step, blob, want in (("good", data, 1), ("all bad", all_flipped(data, piece, 604), 0),
                             ("good again", data, 1)):
        files = write_storage(tmp_path, blob, sizes)
        assert verdicts(blob, piece, hashes) == [want] * n
        same(run(g, mode, files, piece, hashes, None, which), [want] * n, f"{mode} {step}")

    seed, sizes = STALE_TWO
    data = b"".join(storage(sizes, seed))
    hashes = digests(data, piece)
    n = len(hashes) // 20
    two = tmp_path / "two"
    two.mkdir()
    files = write_storage(two, data, sizes)
    which = random.Random(603).sample(range(n), n) if mode == "which" else None
    pick = (lambda v: [v[i] for i in which]) if which else list
    same(run(g, mode, files, piece, hashes, None, which), [1] * n, f"{mode} two files")
    os.unlink(files[1][0])
    lost = sizes[0] // piece                      # the first piece with a byte in file 1
    want = [1] * lost + [0] * (n - lost)
    assert host_verdicts(files, piece, hashes) == want
    same(run(g, mode, files, piece, hashes, None, which), pick(want), f"{mode} file 1 unlinked")
    if mode == "which":
        inside = random.Random(605).sample(range(lost), lost)     # wholly in file 0
        same(run(g, mode, files, piece, hashes, None, inside), [1] * lost, "pieces of file 0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [pytest.param(n, id=f"{n}-seed{DIFF[n]['seed']}") for n in DIFF])
def test_verdicts_match_the_host_under_tampering(tmp_path, name):
    """Data and hash list both tampered with: every device path gives hashlib's verdicts, which
    are the host verify_pieces' too - with `which` unsorted and with duplicates as well."""
    geo = DIFF[name]
    piece, chunk = geo["piece"], geo["chunk"]
    data, hashes, want, which, _ = diff_table(name)
    files = write_storage(tmp_path, data, geo["sizes"])
    want = list(want)
    sub = [want[i] for i in which]
    assert verdicts(data, piece, hashes) == want
    assert host_verdicts(files, piece, hashes) == want
    assert host_verdicts(files, piece, hashes, which) == sub
    g = _gpuhash().GpuVerifier(0, geo["slot"], 2)
    same(run(g, "files", files, piece, hashes), want, "verify_files")
    same(run(g, "streamed", files, piece, hashes, chunk), want, "verify_files_streamed")
    same(run(g, "which", files, piece, hashes, chunk, which), sub, "verify_files_streamed, which")
    same(run(g, "files", files, piece, hashes), want, "verify_files after the streamed calls")
    if name == FRONT_END:
        from downloader_amd.ops import hashing
        same(hashing.verify_pieces(files, piece, hashes, backend="gpu"), want, "front end")
        same(hashing.verify_pieces(files, piece, hashes, which=which, backend="gpu"), sub,
             "front end, which")


@pytest.mark.gpu
def test_out_of_range_which_stays_as_it_is(lanes64, tmp_path):
    """ValueError on the device path, 0 on the host - neither changes here."""
    data, good, _ = short_last_table(0)
    files = write_storage(tmp_path, data, (len(data),))
    for which in ([6], [0, -1], [0, 1 << 20]):
        with pytest.raises(ValueError):
            lanes64.verify_files_streamed(files, SHORT_PIECE, good, 256, which=which)
    assert host_verdicts(files, SHORT_PIECE, good, [0, 6, 5]) == [1, 0, 1]
    assert run(lanes64, "which", files, SHORT_PIECE, good, 256, [0, 5]) == [1, 1]
