"""The integer decisions around the fused FK kernels (smplpp_amd/csrc/fk_plan.h) without a GPU.  tests/cpp/fk_plan_dump.cpp, built
here with the address and undefined-behaviour sanitizers, sweeps every plan function and prints one row per input; a sanitizer
report ends it with a non-zero status.

The sweep of the work split: cus in {8, 64, 104, 256, 304}, nvg in {1..20, 107, 108, 109, 512}, nft in {1..9, 16, 40}, with and
without the levelling of the grid.  The rows are checked against what defines them — a partition of every XCD's items, every
(frame tile, vertex group) exactly once, frame tile major, prefetch targets inside the XCD's groups — and, for the split, the three
grids, the three batch cuts, the workspace sizes and the fp32 form's launch, held to tests/golden/fk_plan.json: row counts and
SHA-256 digests of the same rows printed by the expressions of skin_e.hip, skin_h.hip, skin_b.hip and fk.hip as they stood before
the plan was split out (those lines pasted unchanged into a throwaway main).  The digests are data: they are never regenerated from
fk_plan.h.  The b form's cut is held to them where that cut's G' descriptor size did not wrap (V >= 96); below, it now carries the
cap of the other two forms, asserted on its own."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

# layout.h
NJ, KP = 24, 220
HB_KS, HB_A_BYTES, HB_G_BYTES = 14, 4 * 1024, 72 * 1024
BB_KS, BB_A_BYTES = 14, 6 * 1024
G_TILE = 64 * NJ * 48  # G' of one 64-frame tile, every form: E_G_BYTES, HB_G_BYTES, B_LDS_G
MAX_OFFSET = 0x7FFFFF00  # what a 32-bit buffer offset of the kernels may reach
CUS = (8, 64, 104, 256, 304)
NVG = tuple(range(1, 21)) + (107, 108, 109, 512)
NFT = tuple(range(1, 10)) + (16, 40)
COMBOS = len(CUS) * len(NVG) * len(NFT)
ITEMS = len(CUS) * sum(NVG) * sum(NFT)  # (frame tile, vertex group) pairs of the whole sweep


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fk_plan") / "fk_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "fk_plan_dump.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "fk_plan.json")) as f:
        return json.load(f)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr  # a sanitizer report is a failure
    return r.stdout


def digest(text):
    return {"rows": text.count("\n"), "sha256": hashlib.sha256(text.encode()).hexdigest()}


def table(text, cols):
    return np.array(text.split(), np.int64).reshape(-1, cols)


def test_header_is_plain_cpp():
    path = os.path.join(ROOT, "smplpp_amd", "csrc", "fk_plan.h")
    src = open(path).read()
    assert "hip_runtime" not in src and "__global__" not in src
    assert [ln for ln in src.splitlines() if ln.startswith('#include "')] == ['#include "layout.h"']
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True, input='#include "%s"\n' % path)


@pytest.mark.parametrize("mode", ["grid", "split", "ws", "vplan", "cut e", "cut h"])
def test_plans_equal_the_lines_they_replace(dump_exe, golden, mode):
    assert digest(run(dump_exe, *mode.split())) == golden[mode.replace(" ", "_")]


def _uncapped(V):
    return (MAX_OFFSET // (V * 12)) & ~63


def test_b_cut_equals_the_lines_it_replaces_where_they_did_not_wrap_and_is_capped_below(dump_exe, golden):
    lines = run(dump_exe, "cut", "b").splitlines(True)
    # the cut b had: frames by the vertex bytes alone.  Its kernel's G' descriptor size, nft * G_TILE as a 32-bit int, stays in range
    # while (per / 64) * G_TILE does
    kept = [ln for ln in lines if (_uncapped(int(ln.split()[1])) // 64) * G_TILE <= MAX_OFFSET]
    assert digest("".join(kept)) == golden["cut_b"]
    capped = [ln.split() for ln in lines if ln not in kept]
    assert [int(r[1]) for r in capped] == list(range(1, 96))
    for _, V, per in capped:
        assert int(per) == (MAX_OFFSET // G_TILE) * 64 < _uncapped(int(V))  # 1864128 frames: the cap of e and h


@pytest.mark.parametrize("form", "ehb")
def test_batch_cut(dump_exe, form):
    t = table(run(dump_exe, "cut", form).replace(form, "0"), 3)[:, 1:]
    V, per = t[:, 0], t[:, 1]
    assert {1, 61, 6890, 2796202, 2796203} <= set(V.tolist()) and V.min() == 1
    assert (per % 64 == 0).all()
    assert (per * V * 12 <= MAX_OFFSET).all() and ((per // 64) * G_TILE <= MAX_OFFSET).all()
    fits = (64 * V * 12 <= MAX_OFFSET) & (G_TILE <= MAX_OFFSET)  # one 64-frame launch
    assert np.array_equal(per == 0, ~fits)
    assert per[V == 2796202] == 64 and per[V == 2796203] == 0 and (per[V > 2796203] == 0).all()  # either side of the refusal
    assert per[V == 6890] == (MAX_OFFSET // (6890 * 12)) // 64 * 64 == 25920
    # no longer launch would fit: 64 frames more break one of the two bounds
    more = per[per > 0] + 64
    assert ((more * V[per > 0] * 12 > MAX_OFFSET) | ((more // 64) * G_TILE > MAX_OFFSET)).all()


def test_grid(dump_exe):
    g = table(run(dump_exe, "grid"), 6)
    assert len(g) == COMBOS and len({tuple(r[:3]) for r in g.tolist()}) == COMBOS
    cus = g[:, 0]
    for col in (3, 4, 5):
        assert (g[:, col] >= 1).all() and (g[:, col] <= np.maximum(1, cus // 8)).all()
    assert (g[:, 3] <= g[:, 5]).all() and (g[:, 3] < g[:, 5]).any()  # levelling only ever takes workgroups away, and does
    # with levelling the longest run is as long as without it
    longest = []
    for level in (0, 1):
        s = table(run(dump_exe, "split", level), 9)
        key = (s[:, 0] * 1000 + s[:, 1]) * 100 + s[:, 2]
        order = np.argsort(key, kind="stable")
        ks, starts = np.unique(key[order], return_index=True)
        longest.append((ks, np.maximum.reduceat((s[:, 8] - s[:, 7])[order], starts)))
    assert np.array_equal(longest[0][0], longest[1][0]) and np.array_equal(longest[0][1], longest[1][1])


@pytest.mark.parametrize("level", [0, 1])
def test_runs_partition_every_xcds_items(dump_exe, level):
    s = table(run(dump_exe, "split", level), 9)
    cus, nvg, nft, block, vg0, vg1, nvx, i0, i1 = s.T
    xcd, jb = block & 7, block >> 3
    assert np.array_equal(vg0, (xcd * nvg) >> 3) and np.array_equal(vg1, ((xcd + 1) * nvg) >> 3) and np.array_equal(nvx, vg1 - vg0)
    assert (nvx * nft < 2**26).all() and ((jb + 1) * nvx * nft < 2**32).all()  # the unsigned products of the cut do not wrap
    assert (i0 <= i1).all() and (i0 >= 0).all()
    assert (nvx == 0).any() and (i0[nvx == 0] == i1[nvx == 0]).all()  # nvg < 8: an XCD without a group has only empty runs
    # per (cus, nvg, nft, XCD), by workgroup: the runs follow each other from 0 to nvx * nft
    order = np.lexsort((jb, xcd, nft, nvg, cus))
    o = {k: v[order] for k, v in dict(cus=cus, nvg=nvg, nft=nft, xcd=xcd, jb=jb, i0=i0, i1=i1, cnt=nvx * nft).items()}
    first = o["jb"] == 0
    last = np.append(first[1:], True)
    assert len(s) > 0 and first.sum() == COMBOS * 8 == last.sum()
    assert (o["i0"][first] == 0).all() and np.array_equal(o["i1"][last], o["cnt"][last])
    assert np.array_equal(o["i1"][~last], o["i0"][1:][~last[:-1]])


@pytest.mark.parametrize("level", [0, 1])
def test_run_loop_visits_every_item_once_frame_tile_major(dump_exe, level):
    w = table(run(dump_exe, "walk", level), 8)
    cus, nvg, nft, block, k, ft, vg, nxt = w.T
    assert len(w) == ITEMS
    assert (ft >= 0).all() and (ft < nft).all() and (vg >= 0).all() and (vg < nvg).all()
    assert len(np.unique((((cus * 1000 + nvg) * 100 + nft) * 100 + ft) * 1000 + vg)) == ITEMS  # every (ft, vg) of every grid, exactly once
    xcd = block & 7
    vg0, vg1 = (xcd * nvg) >> 3, ((xcd + 1) * nvg) >> 3
    nvx = vg1 - vg0
    assert np.array_equal(ft, k // nvx) and np.array_equal(vg, vg0 + k % nvx)  # frame tile major inside the XCD's groups
    assert (nxt >= vg0).all() and (nxt < vg1).all()
    # a run's rows are consecutive items; each names the next row's group as its prefetch target, the run's last one its own
    same_run = (np.diff(cus) == 0) & (np.diff(nvg) == 0) & (np.diff(nft) == 0) & (np.diff(block) == 0)
    assert (np.diff(k)[same_run] == 1).all() and (np.diff(ft)[same_run] >= 0).all()
    assert np.array_equal(nxt[:-1][same_run], vg[1:][same_run])
    ends = np.append(~same_run, True)
    assert np.array_equal(nxt[ends], vg[ends])


def test_interleaved_lists_visit_every_item_once(dump_exe):
    w = table(run(dump_exe, "items"), 8)
    cus, nvg, nft, block, t, vg, ft, nxt = w.T
    assert len(w) == ITEMS
    assert (ft >= 0).all() and (ft < nft).all() and (vg >= 0).all() and (vg < nvg).all()
    assert len(np.unique((((cus * 1000 + nvg) * 100 + nft) * 100 + ft) * 1000 + vg)) == ITEMS
    xcd, jb = block & 7, block >> 3
    vg0, vg1 = (xcd * nvg) >> 3, ((xcd + 1) * nvg) >> 3
    assert np.array_equal(vg, vg0 + t // nft) and np.array_equal(ft, t % nft) and (vg < vg1).all()  # vertex group major
    same_list = (np.diff(cus) == 0) & (np.diff(nvg) == 0) & (np.diff(nft) == 0) & (np.diff(block) == 0)
    starts = np.append(True, ~same_list)
    assert np.array_equal(t[starts], jb[starts])
    assert np.array_equal(nxt[:-1][same_list], t[1:][same_list])  # the prefetched item is the list's next one ...
    ends = np.append(~same_list, True)
    assert np.array_equal(nxt[ends], t[ends])  # ... or, at its end, the same one again
    stride = np.diff(t)[same_list]
    assert (stride >= 1).all() and (stride <= np.maximum(1, cus[1:][same_list] // 8)).all()


def test_crossing_run(dump_exe):
    """256 CUs, the synthetic model's 108 vertex groups, 257 frames (tests/fk_bits_cases.py): in an XCD with 13 groups and in one with
    14, some workgroup's run crosses a frame tile boundary, so the GPU cases reach the kernels' reload path."""
    s = table(run(dump_exe, "split"), 9)
    s = s[(s[:, 0] == 256) & (s[:, 1] == 108) & (s[:, 2] == (257 + 63) // 64)]
    assert len(s) and set(s[:, 6].tolist()) == {13, 14}
    for groups in (13, 14):
        r = s[(s[:, 6] == groups) & (s[:, 7] < s[:, 8])]
        assert (r[:, 7] // groups != (r[:, 8] - 1) // groups).any()


def test_workspace_plan_covers_what_the_kernels_index(dump_exe):
    text = run(dump_exe, "ws")
    rows = [ln.split() for ln in text.splitlines()]
    assert len(rows) == 4 * 2 * 209
    for form, *v in rows:
        n, rot_in, Gp, A2h, G2h, A3, AT, root, ldA, gp_off, gp_bytes, at_pad = (int(x) for x in v)
        tiles = (n + 63) // 64
        # every form's pose step writes G' of n frames; e and b DMA whole tiles of it, v zeroes the last tile's padding and reads it
        assert Gp >= (n * NJ * 48 if form == "h" else tiles * G_TILE)
        assert root >= (4 * n * (NJ + 1) * 3 if rot_in else 0)
        assert A2h >= (tiles * HB_KS * HB_A_BYTES if form == "h" else 0) and G2h >= (tiles * HB_G_BYTES if form == "h" else 0)
        assert A3 >= (tiles * BB_KS * BB_A_BYTES if form in "eb" else 0)
        if form == "v":
            FT = 1 if n <= 32 else 2  # skin_kernel<FT> reads rows [0, 32 FT ceil(n / 32 FT)) of each of AT's KP columns
            assert ldA >= 32 * FT * ((n + 32 * FT - 1) // (32 * FT)) and AT >= 4 * KP * ldA
            # the zeroed ranges are exactly the padding: G' of frames [n, 64 tiles), rows [n, ldA) of AT
            assert (gp_off, gp_bytes) == ((n * NJ * 12, 4 * (64 * tiles - n) * NJ * 12) if n % 64 else (0, 0))
            assert 4 * gp_off + gp_bytes <= Gp and at_pad == KP * (ldA - n)
        else:
            assert (AT, ldA, gp_off, gp_bytes, at_pad) == (0, 0, 0, 0, 0)


def test_v_plan_covers_the_batch(dump_exe):
    t = table(run(dump_exe, "vplan"), 7)
    n, VGn, FT, nft, nq, grid, shmem = t.T
    assert np.array_equal(FT, np.where(n <= 32, 1, 2))
    assert (32 * FT * nft >= n).all() and (32 * FT * (nft - 1) < n).all()
    assert (4 * nq >= VGn).all() and (4 * (nq - 1) < VGn).all()
    # workgroup b computes vertex quad (b / 8 / nft) * 8 + b % 8 against frame tile b / 8 % nft: every (quad, tile) has one
    assert (grid % (8 * nft) == 0).all() and (grid // nft >= nq).all() and (grid // nft - 8 < nq).all()
    assert np.array_equal(shmem, 4 * 32 * FT * (NJ * 12 + 3))  # G' [32 FT][24][12] + root translations [32 FT][3], fp32


def test_launch_form(dump_exe):
    t = table(run(dump_exe, "form"), 5)
    assert len(t) == 4 * 2 * 3 * 5
    for form, form_ik, slot, override, got in t.tolist():
        assert got == (override or (form_ik if slot == 2 else form))  # layout.h: RANGE_INTERNAL = 2
