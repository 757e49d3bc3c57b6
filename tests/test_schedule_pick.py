"""The measured schedule choice's bookkeeping (csrc/p3d_frame_config.h: SchedulePick), compiled for the host and driven
frame by frame the way p3d_render.cpp drives it.  The expected sequences are the rule itself: every available candidate
runs twice, the second time timed; the fastest stays; a new configuration starts over (CPU only)."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import REPO

SRC = r"""
#include "p3d_frame_config.h"
using namespace p3d;
static SchedulePick pk;
static PickKey key_of(int res_x) { FrameConfig c; c.res_x = res_x; c.res_y = 90; c.max_depth = 4; return pick_key(c); }
extern "C" {
void reset() { pk = SchedulePick(); }
// one frame: returns cand | timed << 8 | decided << 9.  elapsed: what the previous (timed) frame took
int frame(int res_x, int nc, int avail_mask, float elapsed, int ran_as_chosen) {
    const bool avail[3] = {(avail_mask & 1) != 0, (avail_mask & 2) != 0, (avail_mask & 4) != 0};
    pk.begin(key_of(res_x));
    if (pk.pending() >= 0) pk.collect(elapsed);
    const SchedulePick::Next n = pk.next(nc, avail);
    if (n.timed) pk.enqueued(n.cand, ran_as_chosen != 0);
    return n.cand | (n.timed ? 256 : 0) | (n.decided ? 512 : 0);
}
void adopt(int res_x, int cand, int nc) { pk.adopt(key_of(res_x), cand, nc); }
int known(int res_x, int nc) { return pk.measured(key_of(res_x), nc) ? pk.best : -1; }
}
"""
WAVEFRONT, TREE, TILE = 0, 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("pick")
    (d / "pick.cpp").write_text(SRC)
    inc = ["-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "u_4a_2s_p3d_raytracer_template2_amd", "csrc")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC"] + inc + [str(d / "pick.cpp"), "-o", str(d / "pick.so")])
    L = C.CDLL(str(d / "pick.so"))
    L.frame.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]
    return L


def run(L, n, ms, nc, mask, res_x=160, pushed=()):
    """n frames; ms[c] is what candidate c's timed frame takes; the frames in `pushed` end up on another schedule than the
    one chosen.  Returns [(cand, timed, decided)]."""
    out, last = [], -1
    for i in range(n):
        r = L.frame(res_x, nc, mask, ms[last] if last >= 0 else 0.0, 0 if i in pushed else 1)
        out.append((r & 255, bool(r & 256), bool(r & 512)))
        last = (r & 255) if (r & 256) and i not in pushed else -1
    return out


def test_every_candidate_runs_twice_the_second_time_timed_and_the_fastest_stays(lib):
    lib.reset()
    ms = [5.0, 4.0, 3.0, 6.0, 2.0, 7.0]
    got = run(lib, 14, ms, 6, 7)
    assert got[:12] == [(c, t, False) for c in range(6) for t in (False, True)]
    assert got[12:] == [(4, False, True), (4, False, False)]
    assert lib.known(160, 6) == 4 and lib.known(161, 6) == -1


def test_unavailable_candidates_are_skipped_and_cannot_win(lib):
    lib.reset()
    got = run(lib, 9, [1.0, 0.1, 3.0, 2.0, 0.1, 4.0], 6, 5)                 # no tree (features with random draws)
    assert [g[0] for g in got[:8]] == [0, 0, 2, 2, 3, 3, 5, 5] and got[8] == (0, False, True)
    lib.reset()
    assert run(lib, 2, [0.0] * 6, 3, 0) == [(TREE, False, True), (TREE, False, False)]     # nothing fits: tile -> wavefront -> tree
    lib.reset()                                                            # the tile frame was pushed onto another schedule
    got = run(lib, 7, [2.0, 3.0, 1.0], 3, 7, pushed={5})
    assert got[6] == (WAVEFRONT, False, True)


def test_a_new_configuration_starts_over_and_a_tuned_choice_is_adopted(lib):
    lib.reset()
    assert [g[:2] for g in run(lib, 3, [1.0] * 6, 3, 7)] == [(0, False), (0, True), (1, False)]
    assert [g[:2] for g in run(lib, 2, [1.0] * 6, 3, 7, res_x=320)] == [(0, False), (0, True)]
    lib.adopt(640, 4, 6)
    assert lib.known(640, 6) == 4
    assert run(lib, 2, [1.0] * 6, 6, 7, res_x=640) == [(4, False, False)] * 2
    lib.adopt(640, 4, 3)                                                   # a candidate this configuration has not: tile
    assert lib.known(640, 3) == TILE
