"""csrc/pong_band_span.h: the table of chunk columns a single point changes in the score band, which crl_create builds for the raw
delta writer.  The header is pure host C++; tests/band_span_main.cpp calls it from a program of its own, built here with the host
compiler under -fsanitize=address,undefined (nothing is loaded into Python), and its printed table is compared with numpy's
``atlas[a, b] != atlas[c, d]`` column spans: all 924 one-point transitions of the shipped atlas, then a synthetic atlas with an
identical successor, a difference in the first and the last pixel column, and a pixel whose three bytes straddle two chunks."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY, WHOLE = (255, 0), (0, 255)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("band_span") / "band_span_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "competitive_rl_amd", "csrc"), os.path.join(ROOT, "tests", "band_span_main.cpp"), "-o", exe])
    return exe


def run(program, atlas, ink, tmp_path):
    s, s2, rows, width = atlas.shape
    assert s == s2 and atlas.dtype == np.uint8
    f = tmp_path / "atlas.bin"
    atlas.tofile(f)
    p = subprocess.run([program, str(f), str(s), str(rows), str(width), str(ink[0]), str(ink[1])], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-2000:])
    lines = p.stdout.split("\n")
    assert lines[-2].startswith("status ") and lines[-1] == ""
    table = {}
    for ln in lines[:-2]:
        a, b, k, c0, c1 = map(int, ln.split())
        table[a, b, k] = (c0, c1)
    assert len(table) == s * s * 2
    return table, int(lines[-2].split()[1])


def numpy_span(atlas, a, b, c, d):
    """first and last 16-byte chunk of the RGB row in which the band images of (a, b) and (c, d) differ on any row; None: equal"""
    diff = np.repeat((atlas[a, b] != atlas[c, d]).any(0), 3)  # pixel x holds bytes 3x .. 3x + 2
    cols = np.nonzero(diff.reshape(-1, 16).any(1))[0]
    return (int(cols[0]), int(cols[-1])) if len(cols) else None


def ink_rows(atlas):
    rows = np.nonzero((atlas != 255).any(axis=(0, 1, 3)))[0]
    return (int(rows[0]), int(rows[-1]) + 1) if len(rows) else (0, 0)


def check(table, atlas):
    s = atlas.shape[0]
    transitions = 0
    for a in range(s):
        for b in range(s):
            for k, (c, d) in enumerate(((a + 1, b), (a, b + 1))):
                if c >= s or d >= s:
                    assert table[a, b, k] == WHOLE, (a, b, k)
                    continue
                transitions += 1
                want = numpy_span(atlas, a, b, c, d)
                assert table[a, b, k] == (EMPTY if want is None else want), (a, b, k, table[a, b, k], want)
    return transitions


def test_shipped_atlas(program, atlas, tmp_path):
    assert atlas.shape == (22, 22, 34, 160)
    table, status = run(program, atlas, ink_rows(atlas), tmp_path)
    assert status == 0
    assert check(table, atlas) == 924
    widths = [c1 - c0 + 1 for (c0, c1) in table.values() if c1 < 30 and c0 <= c1]
    print("columns per transition: min %d mean %.2f max %d" % (min(widths), np.mean(widths), max(widths)))
    assert max(widths) <= 30 and len(widths) == 924  # (every point changes the shipped band somewhere)


def test_synthetic_atlas(program, tmp_path):
    a = np.full((3, 3, 6, 160), 255, np.uint8)
    a[:, :, 2, 40] = 0  # ink common to every image: rows [2, 5) hold ink
    a[:, :, 4, 41] = 7
    a[0, 1, 3, 0] = 1  # (0, 0) -> (0, 1): the first and the last pixel column
    a[0, 1, 4, 159] = 2
    a[1, 0] = a[0, 0]  # (0, 0) -> (1, 0): an identical successor
    a[1, 1, 2, 5] = 9  # (1, 0) -> (1, 1): one pixel, bytes 15..17: chunks 0 and 1
    a[2, 1, 3, 100] = 3  # (1, 1) -> (2, 1): pixels 5 and 100 -> chunks 0 .. 18
    ink = ink_rows(a)
    assert ink == (2, 5)
    table, status = run(program, a, ink, tmp_path)
    assert status == 0
    assert check(table, a) == 12
    assert table[0, 0, 1] == (0, 29) and table[0, 0, 0] == EMPTY and table[1, 0, 1] == (0, 1) and table[1, 1, 0] == (0, 18)
    assert table[2, 2, 0] == WHOLE and table[2, 2, 1] == WHOLE and table[2, 0, 0] == WHOLE and table[0, 2, 1] == WHOLE
    # a difference outside the ink rows the caller names is reported: 1 + the index of the first such entry, marked whole band
    table, status = run(program, a, (3, 5), tmp_path)
    assert (a[0, 1, 2] != a[1, 1, 2]).any() and not (a[0, 0, :3] != a[1, 0, :3]).any() and not (a[0, 0, :3] != a[0, 1, :3]).any()
    assert status == 1 + (0 * 3 + 1) * 2 + 0 and table[0, 1, 0] == WHOLE  # (0, 1) -> (1, 1) is the first entry that differs in row 2
