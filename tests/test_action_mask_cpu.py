"""The body of csrc/sf_action_mask.hpp — the text k_action_mask compiles — on the CPU against the truth, in the stand-alone
program tests/action_mask/mask_main.cpp, built once plain and once with -fsanitize=address,undefined.  Nothing sanitized is
loaded into Python.

The program computes, for every arena, agent and command, (a) the mask by the header's body over heap buffers of exactly the
documented sizes and (b) the truth by the product's own Core<WaveEmu, ..>::load -> obey -> store on a copy of the state, and
compares them; it also checks the action words of three action strings (the bots' nine, the full table, 32 characters with
repeats), each alone and beside the command words.  The states: the oracle's dumps of every case at its last moment (the
large-pool case among them: 65 zombie slots and 65 exits, the first word of each in use and the second not), and a synthetic
state of edge values: coordinates 0 and N - 1 / M - 1, floor 2, every selection, counts 0 / 1 / 65535, stamina exactly at and one
below a cost, Hp 0."""
import numpy as np
import pytest

import action_mask_cases as mc


def run_both(state, A, n_agents):
    out = {}
    for build in mc.BUILDS:
        rc, text, mask, truth = mc.run_program(state, A, n_agents, build)
        assert rc == 0 and "mask_main ok" in text, (build, text[-4000:])
        assert np.array_equal(mask, truth), build
        out[build] = truth
    assert np.array_equal(out["plain"], out["sanitized"])
    return out["plain"]


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_states(name):
    c = mc.case(name)
    k, dumps, truth = mc.oracle_moments(name)[-1]
    got = run_both(mc.pack(dumps, c.w), len(dumps), c.w.cfg.n_agents)
    assert np.array_equal(got, truth)


def test_large_pools_words_partly_in_use():
    c = mc.case("large")
    _, dumps, _ = mc.oracle_moments("large")[-1]
    map_pidx = [int(c.w.cfg.map_portal[i]) for i in range(c.w.cells)]
    enc = [mc.pack_arena(d, c.w.cfg, map_pidx) for d in dumps]
    assert c.w.cfg.cap_zombies == 65 and c.w.cfg.cap_portals == 65
    assert all(e["scal"][mc.SC_PWN] == 1 for e in enc)  # the second exit word is not in use: its slot counts as free
    # arena 0 with its zombie table empty (no word in use), arena 1 with slot 64 alive beside the player and both words in use
    enc[0]["zom"][:] = 0
    enc[0]["scal"][mc.SC_ZWN] = 0
    h = dumps[1].humans[0]
    enc[1]["zom"][:, 64] = [(h.f << 20) | (h.r << 10) | (h.c + 1) | (1 << 31), 400, 100]
    enc[1]["scal"][mc.SC_ZWN] = 2
    got = run_both(mc.pack_encoded(enc, c.w), len(enc), 1)
    assert not got[1, 0] >> mc.COMMANDS.index("d") & 1  # the zombie of the second word blocks the step


VEC_SEL = [(-1, -1), (-1, 3), (-1, 7)] + [(0, k) for k in range(4)] + [(1, k) for k in range(4)] + [(2, k) for k in range(8)]


def test_synthetic_edge_values():
    c = mc.case("floors")  # three floors of 5 x 6 cells, one commanded human
    cfg = c.w.cfg
    _, dumps, _ = mc.oracle_moments("floors")[0]
    map_pidx = [int(cfg.map_portal[i]) for i in range(c.w.cells)]
    base = mc.pack_arena(dumps[0], cfg, map_pidx)
    N, M = cfg.rows, cfg.cols
    corners = [(0, 0, 0), (2, N - 1, M - 1), (2, 0, M - 1), (1, N - 1, 0), (0, 2, 3), (2, 1, 1)]
    counts = [0, 1, 65535]
    enc = []
    for i, (vec, sel) in enumerate(VEC_SEL):
        # the stamina cost of what is selected: exactly enough, and one short of it
        cost = -cfg.items.thr[sel][0] if vec == 1 else -cfg.items.weapon[sel][0] if vec == 2 else 30
        for short in (0, 1):
            e = {k: v.copy() for k, v in base.items()}
            n = len(enc)
            f, r, col = corners[n % len(corners)]
            fl = (1 + n % 4) | (1 << 3) | mc.HF_ALIVE | mc.HF_CTRL | mc.HF_OCC | ((vec + 1) << 16) | ((sel + 1) << 18)
            cnt = [counts[(n + j) % 3] for j in range(8)]
            hp = [0, 1, 1000, 0xFFFFFFFB][n % 4]
            bpk = [0, 1, 255][n % 3] | ([1, 0, 255][n % 3] << 8) | ([0, 0, 3, 255][(n // 2) % 4] << 16)
            e["hum"][:, 0] = [(f << 20) | (r << 10) | col, fl, hp, cost - short, 100, 0, 0, 0, cnt[0] | (cnt[1] << 16),
                              cnt[2] | (cnt[3] << 16), cnt[4] | (cnt[5] << 16), cnt[6] | (cnt[7] << 16), bpk]
            enc.append(e)
    w = mc.case("floors").w
    A = len(enc)
    got = run_both(mc.pack_encoded(enc, w), A, 1)
    x = mc.COMMANDS.index("x")
    for n in range(A):
        vec, sel = VEC_SEL[n // 2]
        f, r, col = corners[n % len(corners)]
        way = 1 + n % 4
        rr, cc = r + (1, 0, -1, 0)[way - 1], col + (0, 1, 0, -1)[way - 1]
        if vec >= 1 and 0 <= rr < N and 0 <= cc < M and n % 2 == 1:
            assert not got[n, 0] >> x & 1, n  # one short of the cost: refused
        if vec == 1 and 0 <= rr < N and 0 <= cc < M and n % 2 == 0:
            assert got[n, 0] >> x & 1, n  # exactly the cost: the throw goes (or, at count 0, the selection)
    assert (got & 1).all() and not (got >> 30).any()
