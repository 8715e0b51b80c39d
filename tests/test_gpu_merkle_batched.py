"""MerkleHasher.hash_files / verify_files (ops._gpumerkle): pieces of many files in one device
batch, one sha256_leaf_table launch and one sha256_pairs_fin launch per level - needs a real
MI355X.

The reference is an independent recursive tree over hashlib; equality is bit-exact.
"""
from __future__ import annotations

import os
import random

import pytest

from merkle_batched_ref import (LEAF, blob, flip, mixed_lengths, ordered, ref_nodes, units_of,
                                write_files)

pytestmark = pytest.mark.gpu

PLEN = 65536


@pytest.fixture(scope="module")
def gm():
    from downloader_amd.ops import gpu_available, gpumerkle
    if not gpu_available():
        pytest.fail("HIP device not visible: the GPU test tier must run on a MI355X")
    assert "gfx950" in gpumerkle().arch()
    return gpumerkle()


@pytest.fixture(scope="module")
def hashers(gm):
    """batch_bytes -> hasher; 4 MiB only where one batch has to hold more than 64 leaves."""
    return {bb: gm.MerkleHasher(0, bb, 4) for bb in (64 << 10, 256 << 10, 1 << 20, 4 << 20)}


_nodes = {}


def make(root, lengths, piece_len, tag):
    """Files of `lengths` with seeded contents -> ([(path, length)], reference nodes per file).
    A file's content depends on (tag, index, length) only, so a reference is computed once."""
    datas = [blob(n, (tag, i, n)) for i, n in enumerate(lengths)]
    want = []
    for i, (d, n) in enumerate(zip(datas, lengths)):
        key = (tag, i, n, piece_len)
        if key not in _nodes:
            _nodes[key] = b"".join(ref_nodes(d, piece_len))
        want.append(_nodes[key])
    return write_files(root, datas), want


def ones(files, piece_len, clear=()):
    """All-good verdicts of `files` with the units of the files in `clear` zeroed."""
    return b"".join((b"\x00" if k in clear else b"\x01") * units_of(n, piece_len)
                    for k, (_, n) in enumerate(files))


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("piece_len", [16384, 65536, 1 << 20])
def test_mixed_width_units_in_one_batch(hashers, tmp_path, piece_len, order):
    files, want = make(tmp_path / "m", ordered(mixed_lengths(piece_len), order), piece_len, "mix")
    for bb, h in hashers.items():
        if bb >= piece_len:
            assert h.hash_files(files, piece_len) == b"".join(want), bb


def test_same_content_among_different_neighbours(hashers, tmp_path):
    """A file's nodes do not depend on what lies before and after it in the slot, nor on what an
    earlier batch left there: no lane reads past its own leaf."""
    h = hashers[256 << 10]
    x = 3 * LEAF + 55
    others = [1, 2 * LEAF + 9, 16383, LEAF, 4 * LEAF, 777]
    got = []
    for pos, tag in ((0, "first"), (3, "middle"), (6, "last")):
        lengths = others[:pos] + [x] + others[pos:]
        datas = [blob(n, (tag, i)) for i, n in enumerate(lengths)]
        datas[pos] = blob(x, "the-same-content")
        files = write_files(tmp_path / tag, datas)
        nodes = h.hash_files(files, PLEN)
        assert nodes == b"".join(b"".join(ref_nodes(d, PLEN)) for d in datas), tag
        got.append(nodes[32 * pos:32 * pos + 32])
    assert got[0] == got[1] == got[2] == ref_nodes(blob(x, "the-same-content"), PLEN)[0]


@pytest.mark.parametrize("lengths", [
    [2 * LEAF] * 30 + [4 * LEAF] + [LEAF + 1] * 40 + [3 * LEAF + 5, 4 * LEAF],   # fin_start = 6
    [1] * 60 + [3 * LEAF + 1] + [LEAF] * 70,                                     # width-1 tail
], ids=["70x2+3x4", "130x1+1x4"])
def test_finishing_units_across_a_wave_boundary(hashers, tmp_path, lengths):
    """One 4 MiB batch: the outputs that are finished nodes start inside the first wavefront and
    end in the second (76 pairs, finished from 6 on), or the width-1 tail is 130 digests long.
    The 1 MiB hasher takes the same files in several batches."""
    files, want = make(tmp_path / "w", lengths, PLEN, "wave")
    assert hashers[4 << 20].hash_files(files, PLEN) == b"".join(want)
    assert hashers[1 << 20].hash_files(files, PLEN) == b"".join(want)


def test_last_leaf_lengths_inside_a_multi_file_batch(hashers, tmp_path):
    lengths = [k * LEAF + r for k, r in zip([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3],
                                            [1, 55, 56, 63, 64, 16383, 1, 55, 56, 63, 64, 16383])]
    files, want = make(tmp_path / "t", lengths, PLEN, "tail")
    for bb in (256 << 10, 1 << 20):
        assert hashers[bb].hash_files(files, PLEN) == b"".join(want), bb


@pytest.mark.parametrize("lengths", [
    [5, 9 * PLEN + 3, 60000],            # a large file over three batches, small ones round it
    [3 * PLEN, PLEN],                    # the last unit exactly fills the batch
    [3 * PLEN, LEAF, 3 * LEAF],          # three leaves left, the next unit is four wide
    [1] * 40,                            # closed by the width limit: 16 units to a batch
    [1],
], ids=["span3", "exact-fit", "miss-by-a-leaf", "width-limit", "one-byte"])
def test_batch_edges(hashers, tmp_path, lengths):
    files, want = make(tmp_path / "e", lengths, PLEN, "edge")
    assert hashers[256 << 10].hash_files(files, PLEN) == b"".join(want)


VERIFY_LENGTHS = [1, 3 * PLEN + 100, LEAF, 2 * LEAF + 1, PLEN, PLEN + 1, 55, 4 * LEAF - 1,
                  2 * PLEN, 3 * LEAF + 56, 9 * LEAF, 16385, 63, 5 * LEAF + 7, LEAF - 1, 64,
                  7 * LEAF + 16383, 3 * LEAF, 2, 6 * LEAF]


def test_verify_files(hashers, tmp_path):
    from downloader_amd.torrent import merkle
    h = hashers[256 << 10]
    files, want = make(tmp_path / "v", VERIFY_LENGTHS, PLEN, "verify")
    exp = b"".join(want)
    total = len(exp) // 32
    first = [0]
    for _, n in files:
        first.append(first[-1] + units_of(n, PLEN))
    assert h.verify_files(files, PLEN, exp) == b"\x01" * total

    def agree(got):     # the per-file entry on the same hasher, and the host backend
        assert got == b"".join(h.verify_file(p, n, PLEN, w) for (p, n), w in zip(files, want))
        assert got == merkle.verify_files(files, PLEN, want, backend="cpu")

    rng = random.Random("bit-flips")
    for j, (p, n) in enumerate(files):
        off, bit = rng.randrange(n), rng.randrange(8)
        flip(p, off, bit)
        bad = first[j] + (off // PLEN if n > PLEN else 0)
        assert h.verify_files(files, PLEN, exp) == \
            b"\x01" * bad + b"\x00" + b"\x01" * (total - bad - 1), (j, off, bit)
        flip(p, off, bit)
    assert h.verify_files(files, PLEN, exp) == b"\x01" * total

    # a file longer on disk than `length` is hashed only to `length`
    with open(files[3][0], "ab") as f:
        f.write(b"trailing bytes that are not part of the torrent")
    assert h.verify_files(files, PLEN, exp) == b"\x01" * total
    # short by a few bytes inside its second piece: only piece 0 of the four is covered
    assert files[1][1] == 3 * PLEN + 100
    with open(files[1][0], "r+b") as f:
        f.truncate(2 * PLEN - 5)
    got = h.verify_files(files, PLEN, exp)
    assert got == b"\x01" * 2 + b"\x00" * 3 + b"\x01" * (total - 5)
    agree(got)
    # a missing middle file clears its units, the neighbours stay 1
    os.unlink(files[8][0])
    got = h.verify_files(files, PLEN, exp)
    want_ok = bytearray(ones(files, PLEN, clear={8}))
    want_ok[2:5] = bytes(3)
    assert got == bytes(want_ok) and got[first[7]] == got[first[9]] == 1
    agree(got)
    with pytest.raises(RuntimeError):
        h.hash_files(files, PLEN)
    assert h.hash_files(files[2:8], PLEN) == b"".join(want[2:8])


def test_reuse_of_one_hasher(hashers, tmp_path):
    h = hashers[64 << 10]
    lengths = [3 * LEAF + 1, 2 * PLEN + 9, 1, LEAF, 4 * LEAF, 100]
    files, want = make(tmp_path / "r", lengths, PLEN, "reuse")
    bad_files = write_files(tmp_path / "bad",
                            [blob(n, ("tampered", i)) for i, n in enumerate(lengths)])
    exp = b"".join(want)
    total = len(exp) // 32
    assert h.verify_files(files, PLEN, exp) == b"\x01" * total
    assert h.verify_files(bad_files, PLEN, exp) == bytes(total)
    assert h.verify_file(files[1][0], lengths[1], PLEN, want[1]) == b"\x01" * 3
    assert h.verify_files(files, PLEN, exp) == b"\x01" * total
    assert h.hash_file(files[0][0], lengths[0], PLEN) == (b"", want[0])
    assert h.hash_files(files, PLEN) == exp


def test_three_hundred_small_files_in_one_call(hashers, tmp_path):
    rng = random.Random("small-files")
    lengths = [rng.randint(1, 3 * LEAF) for _ in range(300)]
    files, want = make(tmp_path / "s", lengths, PLEN, "small")
    for bb in (1 << 20, 4 << 20):
        assert hashers[bb].hash_files(files, PLEN) == b"".join(want), bb


def test_argument_errors_leave_the_hasher_working(hashers, tmp_path):
    h = hashers[256 << 10]
    files, want = make(tmp_path / "a", [5 * LEAF, 7], PLEN, "args")
    exp = b"".join(want)
    for bad in (24576, 8192, 1 << 20):       # no power of two, below 16 KiB, above batch_bytes
        with pytest.raises(ValueError):
            h.hash_files(files, bad)
        with pytest.raises(ValueError):
            h.verify_files(files, bad, exp)
    with pytest.raises(ValueError):
        h.hash_files([], PLEN)
    with pytest.raises(ValueError):
        h.verify_files([], PLEN, b"")
    with pytest.raises(ValueError):
        h.hash_files([files[0], (files[1][0], 0)], PLEN)
    with pytest.raises(ValueError):
        h.verify_files([files[0], (files[1][0], -3)], PLEN, exp)
    with pytest.raises(ValueError):
        h.verify_files(files, PLEN, exp[:-32])
    with pytest.raises(ValueError):
        h.verify_files(files, PLEN, exp + bytes(1))
    assert h.verify_files(files, PLEN, exp) == b"\x01" * 3
    assert h.hash_files(files, PLEN) == exp


def test_merkle_module_gpu_backend_equals_cpu(gm, tmp_path):
    from downloader_amd.torrent import merkle
    files, want = make(tmp_path / "p", mixed_lengths(PLEN), PLEN, "mix")
    assert merkle.hash_files(files, PLEN, backend="gpu") == b"".join(want)
    assert merkle.hash_files(files, PLEN, backend="cpu") == b"".join(want)
    flip(files[5][0], 5 * LEAF)
    cpu = merkle.verify_files(files, PLEN, want, backend="cpu")
    assert merkle.verify_files(files, PLEN, want, backend="gpu") == cpu
    assert cpu.count(0) == 1
