"""The batch plan of the BEP 52 device recheck (csrc/merkle_plan.h through _native.merkle_plan)
and the whole-torrent entries of torrent.merkle on the host backend. No device needed: the plan
is carried out here with hashlib, step by step as the device does, against an independent
recursive tree."""
from __future__ import annotations

import json
import os

import pytest

from merkle_batched_ref import (LEAF, ZERO, blob, flip, mixed_lengths, ordered, ref_nodes, sha256,
                                units_of, write_files)

from downloader_amd.ops import native
from downloader_amd.torrent import merkle

PIECE_LENS = [16384, 65536, 1 << 20]
ORDERS = ["ascending", "descending", "shuffled"]


def run_plan(datas, piece_len: int, batch_bytes: int):
    """Carry a plan out the way MerkleHasher does: reads into a slot that holds stale bytes,
    the leaf table into a zeroed level-0 list, one uniform pass per level, finished nodes into
    the result by (fin_start, unit_base), width-1 units from the level-0 tail, then the inverse
    permutation."""
    plan = native().merkle_plan([len(d) for d in datas], piece_len, batch_bytes)
    out = [None] * sum(units_of(len(d), piece_len) for d in datas)
    for b in plan:
        slot = bytearray(b"\xa5" * batch_bytes)
        for f, fo, ln, so in b["reads"]:
            assert so + ln <= batch_bytes
            slot[so:so + ln] = datas[f][fo:fo + ln]
        lvl = [ZERO] * b["width_sum"]
        for src, ln, dst in b["leaves"]:
            lvl[dst] = sha256(bytes(slot[src:src + ln]))
        nu, w1 = len(b["units"]), b["w1_count"]
        res = [None] * nu
        res[nu - w1:] = lvl[b["width_sum"] - w1:]
        for n_pairs, fin_start, unit_base in b["levels"]:
            lvl = [sha256(lvl[2 * i] + lvl[2 * i + 1]) for i in range(n_pairs)]
            for i in range(fin_start, n_pairs):
                res[unit_base + i - fin_start] = lvl[i]
        assert sorted(b["order"]) == list(range(nu))
        for j, u in enumerate(b["order"]):
            assert out[b["first_unit"] + u] is None
            out[b["first_unit"] + u] = res[j]
    return out, plan


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("piece_len", PIECE_LENS)
def test_plan_executed_with_hashlib_matches_the_recursive_tree(piece_len, order):
    lengths = ordered(mixed_lengths(piece_len), order)
    datas = [blob(n, (i, n)) for i, n in enumerate(lengths)]
    want = [x for d in datas for x in ref_nodes(d, piece_len)]
    for batch_bytes in (piece_len, 4 * piece_len, 1 << 22):
        got, plan = run_plan(datas, piece_len, batch_bytes)
        assert got == want, (piece_len, order, batch_bytes)
        if piece_len == 16384:                 # every width 1: no levels at all
            assert all(not b["levels"] and b["w1_count"] == len(b["units"]) for b in plan)


def check_invariants(lengths, piece_len, batch_bytes):
    plan = native().merkle_plan(lengths, piece_len, batch_bytes)
    cap = batch_bytes // LEAF
    seen = set()
    next_unit = 0
    next_piece = {}
    for b in plan:
        assert b["units"], "an empty batch"
        assert b["first_unit"] == next_unit
        next_unit += len(b["units"])
        assert b["data_bytes"] <= batch_bytes
        assert b["width_sum"] == sum(u[2] for u in b["units"]) <= cap
        assert len(b["leaves"]) <= b["width_sum"]
        end = 0
        for f, fo, ln, so in b["reads"]:
            assert so % 256 == 0 and so >= end      # 256-aligned file starts, no overlap
            assert fo % piece_len == 0               # a large file splits at a piece boundary
            assert fo + ln == lengths[f] or (fo + ln) % piece_len == 0
            end = so + ln
        assert end == b["data_bytes"]
        for f, piece, width, so, nbytes in b["units"]:
            assert piece == next_piece.get(f, 0)     # file order, then piece order
            next_piece[f] = piece + 1
            assert width & (width - 1) == 0
            if lengths[f] > piece_len:
                assert width == piece_len // LEAF
                assert nbytes == min(piece_len, lengths[f] - piece * piece_len)
            else:
                assert nbytes == lengths[f] and width // 2 * LEAF < nbytes <= width * LEAF
            rd = [r for r in b["reads"] if r[0] == f]
            assert len(rd) == 1 and so == rd[0][3] + piece * piece_len - rd[0][1]
        dsts = set()
        for src, ln, dst in b["leaves"]:
            assert 1 <= ln <= LEAF and src % 16 == 0 and src + ln <= b["data_bytes"]
            assert 0 <= dst < b["width_sum"] and dst not in dsts
            dsts.add(dst)
            f, fo, _, so = [r for r in b["reads"] if r[3] <= src < r[3] + r[2]][0]
            key = (f, fo + src - so)
            assert key not in seen and key[1] % LEAF == 0
            assert ln == min(LEAF, lengths[f] - key[1])
            seen.add(key)
    assert seen == {(f, o) for f, n in enumerate(lengths) for o in range(0, n, LEAF)}
    assert next_unit == sum(units_of(n, piece_len) for n in lengths)
    return plan


@pytest.mark.parametrize("piece_len,batch_bytes", [(16384, 65536), (65536, 65536),
                                                   (65536, 262144), (1 << 20, 1 << 20),
                                                   (1 << 20, 4 << 20)])
def test_plan_invariants(piece_len, batch_bytes):
    for order in ORDERS:
        check_invariants(ordered(mixed_lengths(piece_len) + [3 * piece_len + 5], order),
                         piece_len, batch_bytes)


def test_plan_width_limit_closes_a_batch_of_one_byte_files():
    plan = check_invariants([1] * 200, 16384, 65536)
    assert len(plan) == 50 and all(len(b["units"]) == 4 for b in plan)
    assert all(b["data_bytes"] == 3 * 256 + 1 for b in plan)
    plan = check_invariants([1] * 200, 65536, 65536)
    assert all(len(b["units"]) <= 4 for b in plan)


def test_plan_unit_of_a_whole_batch_and_near_fits():
    plen = 65536
    plan = check_invariants([plen], plen, plen)
    assert len(plan) == 1 and plan[0]["data_bytes"] == plen
    assert plan[0]["levels"] == [(2, 2, 1), (1, 0, 0)]
    # 256 KiB batch (16 leaves): 3 pieces and a 4-leaf file fill it exactly
    plan = check_invariants([3 * plen, plen], plen, 4 * plen)
    assert [len(b["units"]) for b in plan] == [4]
    assert plan[0]["data_bytes"] == 4 * plen and plan[0]["width_sum"] == 16
    # 13 leaves taken, 3 left: a 3-leaf file is 4 wide and starts the next batch
    plan = check_invariants([3 * plen, LEAF, 3 * LEAF], plen, 4 * plen)
    assert [len(b["units"]) for b in plan] == [4, 1]
    # a large file over three batches with small files round it
    plan = check_invariants([5, 9 * plen + 3, 60000], plen, 4 * plen)
    assert [len(b["units"]) for b in plan] == [4, 4, 4]
    assert [sorted({u[0] for u in b["units"]}) for b in plan] == [[0, 1], [1], [1, 2]]


def test_plan_levels_of_mixed_widths():
    # widths 4, 4, 2, 2, 2, 1 in sorted order: 15 level-0 digests
    lengths = [1, 2 * LEAF, 4 * LEAF, LEAF + 1, 3 * LEAF + 1, 2 * LEAF]
    (b,) = native().merkle_plan(lengths, 65536, 1 << 20)
    assert b["order"] == [2, 4, 1, 3, 5, 0] and b["width_sum"] == 15 and b["w1_count"] == 1
    assert b["levels"] == [(7, 4, 2), (2, 0, 0)]


def test_plan_argument_errors():
    plan = native().merkle_plan
    for lengths, plen, bb in [([], 16384, 65536), ([0], 16384, 65536), ([5, -1], 16384, 65536),
                              ([5], 8192, 65536), ([5], 24576, 65536), ([5], 0, 65536),
                              ([5], 131072, 65536)]:
        with pytest.raises(ValueError):
            plan(lengths, plen, bb)


# -- torrent.merkle on the host backend ---------------------------------------------------------

def make_pack(tmp_path, piece_len):
    from downloader_amd.torrent.metainfo_v2 import make_torrent_v2, parse_torrent_v2
    root = tmp_path / "pack"
    lengths = ordered(mixed_lengths(piece_len), "shuffled")
    write_files(root, [blob(n, ("pack", i)) for i, n in enumerate(lengths)])
    m = parse_torrent_v2(make_torrent_v2(str(root), piece_len))
    local = m.local_files(str(tmp_path))
    assert [n for _, n in local] == lengths
    return root, m, local


@pytest.mark.parametrize("piece_len", [16384, 65536])
def test_verify_files_and_hash_files_cpu_equal_the_per_file_functions(tmp_path, piece_len):
    root, m, local = make_pack(tmp_path, piece_len)
    exp = [m.expected(f) for f in m.files]
    per_file = b"".join(merkle.verify_file(p, n, piece_len, e) for (p, n), e in zip(local, exp))
    ok = merkle.verify_files(local, piece_len, exp, backend="cpu")
    assert ok == per_file == b"\x01" * m.num_pieces
    nodes = merkle.hash_files(local, piece_len, backend="cpu")
    assert nodes == b"".join(exp)
    want = b"".join(b"".join(ref_nodes(open(p, "rb").read(), piece_len)) for p, _ in local)
    assert nodes == want
    first = [0]
    for _, n in local:
        first.append(first[-1] + units_of(n, piece_len))
    # one flipped byte in file j clears exactly that unit
    for j, (p, n) in enumerate(local):
        off = n - 1
        flip(p, off)
        got = merkle.verify_files(local, piece_len, exp, backend="cpu")
        bad = first[j] + (off // piece_len if n > piece_len else 0)
        assert got == b"\x01" * bad + b"\x00" + b"\x01" * (m.num_pieces - bad - 1), j
        flip(p, off)
    # a missing file clears its units only
    j = max(range(len(local)), key=lambda k: local[k][1])
    os.unlink(local[j][0])
    got = merkle.verify_files(local, piece_len, exp, backend="cpu")
    assert got == b"".join(b"\x00" * units_of(n, piece_len) if k == j else
                           b"\x01" * units_of(n, piece_len) for k, (_, n) in enumerate(local))
    with pytest.raises((RuntimeError, OSError)):
        merkle.hash_files(local, piece_len, backend="cpu")


def test_verify_files_argument_errors(tmp_path):
    p = tmp_path / "a.bin"
    p.write_bytes(blob(5 * LEAF, "args"))
    f = [(str(p), 5 * LEAF)]
    for call in (lambda: merkle.verify_files([], 16384, []),
                 lambda: merkle.verify_files(f, 24576, [bytes(32)]),
                 lambda: merkle.verify_files(f, 16384, [bytes(32 * 4)]),
                 lambda: merkle.verify_files(f, 16384, []),
                 lambda: merkle.verify_files([(str(p), 0)], 16384, [b""]),
                 lambda: merkle.verify_files(f, 1 << 20, [bytes(64)]),
                 lambda: merkle.verify_files(f, 16384, [bytes(160)], backend="nope"),
                 lambda: merkle.hash_files([], 16384),
                 lambda: merkle.hash_files([(str(p), -1)], 16384),
                 lambda: merkle.hash_files(f, 8192)):
        with pytest.raises(ValueError):
            call()


def test_cli_verify_v2_exit_codes_and_line(tmp_path, capsys):
    from downloader_amd.__main__ import main
    root, m, local = make_pack(tmp_path, 65536)
    tor = tmp_path / "pack.torrent"
    assert main(["make-torrent", str(root), "-o", str(tor), "--piece-length", "65536",
                 "--meta-version", "2"]) == 0
    capsys.readouterr()
    assert main(["verify", str(tor), str(tmp_path), "--backend", "cpu"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert set(out) == {"pieces", "good", "seconds", "GBps", "backend", "meta_version"}
    assert out["pieces"] == out["good"] == m.num_pieces and out["backend"] == "cpu"
    flip(local[3][0], 0)
    assert main(["verify", str(tor), str(tmp_path), "--backend", "cpu"]) == 1
    out = json.loads(capsys.readouterr().out)
    assert out["pieces"] == m.num_pieces and out["good"] == m.num_pieces - 1
    os.unlink(local[3][0])
    assert main(["verify", str(tor), str(tmp_path), "--backend", "cpu"]) == 1
