"""The reach of the games of tests/record_cases.py, from the oracle alone: together they hold every situation the record
kernels must get right.  These are conditions on the cases, not measurements."""
import record_cases as rc
from strikeforce_amd import abi


def _arenas_with(fact):
    return [(name, a) for name in sorted(rc.CASES) for a, f in enumerate(rc.CASES[name]().facts) if fact in f]


def test_a_dead_players_slot_is_taken_by_a_spawned_npc_while_the_game_runs():
    assert ("squad", 0) in _arenas_with("npc in a dead player's slot")
    p = rc.squad_played()
    g = p.games[0][0]
    # agent 1 had a line up to its quit in iteration 24 and none after, although its slot is alive again later
    reused = [t for t in range(len(p.cmds)) if (p.flags[t, 0, 1] & (rc.HF_ALIVE | rc.HF_CTRL)) == rc.HF_ALIVE]
    assert reused and reused[0] > 24 and g["end"] is None
    assert len(g["stream"]) == 25 * 3 + 3 * 2 + (len(p.cmds) - 28)


def test_ind_dies_in_the_first_half_of_an_iteration_and_its_line_is_written():
    hit = _arenas_with("ind died in the first half")
    assert len([x for x in hit if x[0] == "solo"]) >= 4
    p = rc.solo_played()
    for _, a in hit:
        ended = [g for g in p.games[a] if g["end"] == abi.RECORD_GAME_ENDED]
        assert ended and all(len(g["stream"]) == g["iterations"] and g["outcome"] == abi.DIED for g in ended)


def test_games_end_by_check_end_and_arenas_play_several():
    assert len(_arenas_with("ended by check_end")) >= 12
    two = _arenas_with("two games in one arena")
    assert {n for n, _ in two} == {"fight", "solo"}
    p = rc.fight_played()
    assert p.w.cfg.auto_reset == 1 and all(len(p.games[a]) == 3 for a in range(0, rc.FIGHT_ARENAS, 4))
    # consecutive games of an arena: episodes count up and the seed moves by the reseed stride
    for a in range(0, rc.FIGHT_ARENAS, 4):
        g = p.games[a]
        assert [x["episode"] for x in g] == [0, 1, 2] and [x["tb"] - g[0]["tb"] for x in g] == [0, rc.FIGHT_ARENAS, 2 * rc.FIGHT_ARENAS]
    # with auto_reset off a finished arena stands still
    q = rc.squad_played()
    assert q.games[1][0]["end"] == abi.RECORD_GAME_ENDED and len(q.games[1]) == 1 and q.games[1][0]["iterations"] < len(q.cmds)


def test_command_bytes_no_sample_can_carry():
    assert _arenas_with("substituted") == [("fight", 3), ("fight", 5)]
    p = rc.fight_played()
    fed = {int(c) for c in p.cmds.reshape(-1)}
    assert {0x00, 0x0a, 0x1f, 0x20, 0x7f, 0x80, 0xff} <= fed
    for gs in p.games:
        for g in gs:
            assert all(0x21 <= c <= 0x7e for c in g["stream"])


def test_shapes_and_lengths_stay_small():
    for name in rc.CASES:
        p = rc.CASES[name]()
        assert p.w.cfg.arenas <= 64 and len(p.cmds) <= 120
    assert rc.batch_workload().cfg.arenas == 24 and rc.BATCH_ITERS <= 120
