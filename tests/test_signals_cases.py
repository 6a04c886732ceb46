"""The cases of tests/signals_cases.py reach what the sf_signals_* tests are meant to meet, shown from the restatement over
the oracle alone (no engine): every flag bit, every rule and branch, the outcomes, and the sizes and options the cases must
span.  A device test that compares with the restatement can therefore not pass by never meeting a case."""
import pytest

import signals_cases as sc

EVERY_CASE = {"rule1:first", "flag:REBASED"}
REACH = {
    "timer-k1-k8": {"rule4:present", "rule3:present", "outcome:3", "rule2", "flag:UNRESOLVED", "rule1:whole-reset", "flag:ENDED"},
    "timer-still": {"rule3:present", "outcome:3", "idle", "flag:IDLE"},
    "solo-restarts": {"outcome:1", "rule1:announced", "rule1:seed", "rule1:steps", "rule3:present"},
    "solo-restarts-still": {"outcome:1", "rule1:announced", "rule1:seed", "rule1:steps", "idle", "rule4:absent"},
    "battle3": {"rule4:corpse", "flag:DIED", "rule4:absent", "rule3:absent", "outcome:2", "outcome:1",
                "rule4:gone:slot-empty:steps", "flag:UNRESOLVED"},
    "battle3-still": {"rule4:corpse", "outcome:2", "outcome:1", "rule3:died-in-the-last-step", "idle"},
    "squad3-npc": {"rule4:gone:slot-alive:one-step", "rule4:gone:slot-alive:steps", "rule4:corpse", "flag:UNRESOLVED"},
    "battle16": {"rule4:present", "rule4:corpse", "rule4:absent"},
    "battle16-still": {"rule4:present", "rule4:corpse", "rule4:absent"},
    "snapshot": {"rule1:seed", "rule1:steps", "rule1:announced", "rule4:corpse"},
    "replay-end": {"rule4:newly-done:%d" % sc.SF_SAMPLE_END, "idle", "rule4:present"},
}


@pytest.fixture(scope="module")
def reach():
    return {name: sc.run(sc.case(name)).reach for name in sc.NAMES}


@pytest.mark.parametrize("name", sc.NAMES)
def test_each_case_reaches_what_it_is_there_for(reach, name):
    missing = (REACH[name] | EVERY_CASE) - reach[name]
    assert not missing, (name, sorted(missing), sorted(reach[name]))


def test_every_flag_rule_and_outcome_is_reached(reach):
    union = set().union(*reach.values())
    flags = {"flag:" + f for f in ("PRESENT", "DIED", "ENDED", "REBASED", "UNRESOLVED", "IDLE")}
    rules = {"rule1:first", "rule1:announced", "rule1:whole-reset", "rule1:seed", "rule1:steps", "rule2", "rule3:present",
             "rule3:absent", "rule4:present", "rule4:corpse", "rule4:gone:slot-alive:one-step", "rule4:gone:slot-alive:steps",
             "rule4:gone:slot-empty:steps", "rule4:absent", "rule4:newly-done:6", "idle"}
    outcomes = {"outcome:%d" % o for o in (sc.SF_DIED, sc.SF_WON, sc.SF_TIME_LOST)}  # ('_' ends a game as SF_DIED)
    assert not (flags | rules | outcomes) - union, sorted((flags | rules | outcomes) - union)


def test_the_cases_span_the_sizes_and_options():
    cases = [sc.case(n) for n in sc.NAMES]
    assert {c.w.cfg.arenas for c in cases} == {3, 5}
    assert {c.w.cfg.n_agents for c in cases} == {1, 3, 16}
    assert {c.w.cfg.auto_reset for c in cases} == {0, 1}
    kinds = {op[0] for c in cases for op in c.script}
    assert kinds == {"reset", "step", "many", "signals", "restart", "save", "load", "replay_step"}
    assert any(op[0] == "many" and len(op[1]) == 8 for op in sc.case("timer-k1-k8").script)
    # restarts on a new seed and on the same seed, announced and not; loads announced and not
    restarts = [(isinstance(op[1].get("tb"), str), op[2]) for op in sc.case("solo-restarts").script if op[0] == "restart" and "tb" in op[1]]
    assert set(restarts) == {(False, False), (True, False), (True, True)}
    assert {op[2] for op in sc.case("snapshot").script if op[0] == "load"} == {False, True}


def test_a_k8_launch_ends_two_games_in_one_arena():
    c = sc.case("timer-k1-k8")
    src = sc.make_ref(c)
    try:
        for op in c.script[1:]:
            if op[0] == "step":
                src.step(op[1])
            elif op[0] == "many":
                before = src.episodes()
                for row in op[1]:
                    src.step(row)
                assert ((src.episodes() - before) >= 2).all()
                return
        raise AssertionError("no k-step launch in the script")
    finally:
        src.close()
