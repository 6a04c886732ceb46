"""The restatement of sf_signals_step (tests/signals_ref.py) against sequences derived by hand:
  - a scripted quit: the reference's '_' (gameplay.hpp:696-699) sets the player's Hp to 0, check_end ends the game as
    SF_DIED, so the call behind that step must report ENDED, d Hp = -(the Hp before) and nothing else, and the reward is
    per_step + w_hp * d Hp + outcome[SF_DIED] in float32; the arena then stands still;
  - a scripted kill: in a Squad start every human stands in row 1, slot i at column i + 1, teams 1 (slots 0-4) and 2 (slots
    5-9), all ten commanded and told to stand still; human 4 turns towards human 5 and punches.  Human::punch
    (Character.hpp:391-397) deals max(compute_damage(mindamage_def, 1), mindamage) per hit, the victim has its profile's
    def_hp, so the hits needed, the d damage of every call, the one d kills and the arena's teams_kills / loot (gameplay.hpp:
    625-629: +1 and +100 for a team-mate's kill) are all known beforehand."""
import numpy as np

import signals_cases as sc
from oracle_lib import lib
from reset_sel_ref import ResetSelRef
from signals_ref import DIED, ENDED, IDLE, PRESENT, REBASED, SignalsRef
from strikeforce_amd import abi, config, env

F32 = np.float32


def test_scripted_quit():
    w = config.baseline_workload("C1", arenas=3, auto_reset=0)
    tb, sr = w.seeds()
    src = ResetSelRef(w, tb, sr)
    ref = SignalsRef(src)
    wts = env.reward_weights(per_step=0.3, hp=0.01, died=7.0, outcome={sc.SF_DIED: -1.7})
    try:
        v, d, r = ref.step(None, wts)
        assert (d[:, :, 0] == (REBASED | PRESENT)).all() and not d[:, :, 1:].any() and not r.any()
        hp = v[:, 0, 1].copy()
        assert (hp == w.cfg.player.def_hp).all()
        src.step(np.array([[ord("+")], [ord("_")], [ord("+")]], dtype=np.uint8))
        v, d, r = ref.step(None, wts)
        assert d[1].tolist() == [[ENDED, 0, 0, 0, 0, 0, -hp[1], sc.SF_DIED]] and not v[1, 0, 1:12].any()
        expect = F32(F32(F32(0.3) + F32(F32(0.01) * F32(-hp[1]))) + F32(-1.7))  # the five zero terms add nothing; no DIED flag
        assert r[1, 0].view(np.uint32) == expect.view(np.uint32)
        for a in (0, 2):  # nothing happened to the others in one step
            assert d[a].tolist() == [[PRESENT, 0, 0, 0, 0, 0, 0, 0]] and r[a, 0] == F32(0.3)
        src.step(np.full((3, 1), ord("+"), dtype=np.uint8))
        v, d, r = ref.step(None, wts)
        assert d[1].tolist() == [[IDLE, 0, 0, 0, 0, 0, 0, 0]] and r[1, 0] == 0
        assert ref.status() == (0, 0)
    finally:
        src.close()


def test_scripted_kill():
    cfg = config.make_config(3, 32, 32, H=10, Z=8, B=64, P=8, mode=abi.MODE_SQUAD, n_agents=10, auto_reset=0)
    keep = [(0, 3, 1)] + [(0, 1, i + 1) for i in range(1, 10)]
    w = config.Workload("sig-kill", cfg, *config.synthetic_map(32, 32, wall_p=0.0, keep_clear=keep))
    tb, sr = w.seeds()
    src = ResetSelRef(w, tb, sr)
    ref = SignalsRef(src)
    wts = env.reward_weights(kills=10.0, damage=0.001)
    try:
        v, d, r = ref.step()
        assert [int(x) for x in v[0, 4, 7:12]] == [0, 1, 5, 1, 1] and [int(x) for x in v[0, 5, 7:12]] == [0, 1, 6, 1, 2]
        hit = max(lib().sfo_kat_compute_damage(cfg.npc.mindamage_def, 1), int(v[0, 4, 3]))
        victim_hp = int(v[0, 5, 1])
        assert victim_hp == cfg.npc.def_hp and hit > 0
        need = -(-victim_hp // hit)  # hits until the victim's Hp is <= 0
        row = np.full((3, 10), ord("+"), dtype=np.uint8)
        row[:, 4] = ord("q")  # way 1 (down) -> 2 (right): towards column 6
        src.step(row)
        v, d, r = ref.step(None, wts)
        assert v[0, 4, 10] == 2 and not d[:, :, 1:].any()
        row[:, 4] = ord("z")
        hits, log = 0, []
        for s in range(need + 3):
            src.step(row)
            v, d, r = ref.step(None, wts)
            dk, ddmg = int(d[0, 4, 1]), int(d[0, 4, 4])
            log.append((dk, ddmg))
            assert ddmg in (0, hit), log
            hits += ddmg == hit
            assert int(d[0, 5, 6]) == -ddmg or hits >= need, log  # what human 4 deals is what human 5 loses
            if hits < need:
                assert dk == 0 and d[0, 4, 0] == PRESENT and d[0, 5, 0] == PRESENT, log
            elif ddmg:  # the killing hit: one kill for human 4, one team kill and 100 loot for the arena, human 5 is gone
                assert dk == 1 and [int(x) for x in d[0, 4, 1:4]] == [1, 1, 100], log
                assert [int(x) for x in d[0, 0, 1:4]] == [0, 1, 100]  # `ind` sees the arena's counters, not the kill
                assert d[0, 5, 0] == DIED and not v[0, 5, 1:12].any()
                assert r[0, 4].view(np.uint32) == F32(F32(F32(0.0) + F32(F32(10.0) * F32(1.0))) + F32(F32(0.001) * F32(hit))).view(np.uint32)
                break
        else:
            raise AssertionError(("no kill", log))
        assert hits == need and hits * hit >= victim_hp > (hits - 1) * hit
        assert (d[1] == d[0]).all() and (d[2] == d[0]).all()  # nothing random is in play: every arena tells the same story
    finally:
        src.close()
