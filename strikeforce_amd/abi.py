"""ctypes mirror of include/strikeforce.h (the C-ABI boundary).

Only data layout lives here; the loader for the HIP library is in ``env.py``.  The same structures
are used by ``tests/`` to talk to the CPU oracle, which exports the same calls with an ``sfo_`` prefix.
"""
import ctypes as C

SF_ABI_VERSION = 2
OBS_CHANNELS = 32
OBS_WINDOW = 31
OBS_FLOATS = OBS_CHANNELS * OBS_WINDOW * OBS_WINDOW  # 30752, bots/bot-0.5/Custom.hpp:137-159

MAX_HUMANS = 64
MAX_ZOMBIES = 9000
MAX_BULLETS = 256
MAX_PORTALS = 9000
MAX_AGENTS = 16

MODE_SOLO, MODE_TIMER, MODE_SQUAD, MODE_BATTLE = 0, 1, 2, 3
RUNNING, DIED, WON, TIME_LOST, TIME_WON, QUIT = 0, 1, 2, 3, 4, 5
SAMPLE_END = 6  # SF_SAMPLE_END: a replayed arena whose command stream ran out (sf_replay_step)
REPLAY_RUNNING, REPLAY_GAME_ENDED, REPLAY_SAMPLE_ENDED, REPLAY_TRUNCATED = 0, 1, 2, 3  # SF_REPLAY_*
REPLAY_STATES = ("running", "game ended", "sample ended", "truncated")

CELL_WALL, CELL_TEMP, CELL_PIN_UP, CELL_PIN_DN, CELL_POUT, CELL_CHEST = 1, 2, 4, 8, 16, 32
CELL_CONS_SHIFT = 6

# gameplay.hpp:45 valid_commands plus '_' (gameplay.hpp:696): the 30 command codes.
VALID_COMMANDS = "+qe3uzxawsdfghjkl;'cvbnm,./[]"
ALL_COMMANDS = VALID_COMMANDS + "_"
# bench/random-agent command set: the 30 codes minus the UI toggle '3' and suicide '_'.
BENCH_COMMANDS = "+qeuzxawsdfghjkl;'cvbnm,./[]"
assert len(ALL_COMMANDS) == 30 and len(BENCH_COMMANDS) == 28


class Profile(C.Structure):
    _fields_ = [
        ("def_hp", C.c_int32), ("mindamage_def", C.c_int32), ("def_stamina", C.c_int32),
        ("level_solo", C.c_int32), ("level_timer", C.c_int32), ("level_squad", C.c_int32),
        ("money", C.c_int32),
        ("rate_solo", C.c_int32), ("rate_timer", C.c_int32), ("rate_squad", C.c_int32), ("rate", C.c_int32),
        ("cons", C.c_int32 * 4),
        ("throw_lvl_cnt", (C.c_int32 * 2) * 4),
        ("weapon_lvl", C.c_int32 * 8),
        ("backpack_lvl", C.c_int32),
    ]

    @classmethod
    def from_tokens(cls, tokens):
        """Build from the 32 integers of a reference character file (name token removed)."""
        t = [int(x) for x in tokens]
        if len(t) != 32:
            raise ValueError("a character record has 32 integer tokens after the name, got %d" % len(t))
        p = cls()
        (p.def_hp, p.mindamage_def, p.def_stamina, p.level_solo, p.level_timer, p.level_squad, p.money,
         p.rate_solo, p.rate_timer, p.rate_squad, p.rate) = t[:11]
        for i in range(4):
            p.cons[i] = t[11 + i]
        for i in range(4):
            p.throw_lvl_cnt[i][0] = t[15 + 2 * i]
            p.throw_lvl_cnt[i][1] = t[16 + 2 * i]
        for i in range(8):
            p.weapon_lvl[i] = t[23 + i]
        p.backpack_lvl = t[31]
        return p


class Items(C.Structure):
    _fields_ = [
        ("cons", (C.c_int32 * 3) * 4),
        ("thr", (C.c_int32 * 4) * 4),
        ("weapon", (C.c_int32 * 4) * 8),
    ]


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("arenas", C.c_int32),
        ("floors", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
        ("cap_humans", C.c_int32), ("cap_zombies", C.c_int32), ("cap_bullets", C.c_int32),
        ("cap_portals", C.c_int32), ("cap_chests", C.c_int32),
        ("mode", C.c_int32),
        ("level", C.c_int32),
        ("n_agents", C.c_int32),
        ("ind", C.c_int32),
        ("agent_team", C.c_int32 * MAX_AGENTS),
        ("auto_reset", C.c_int32),
        ("reseed_stride", C.c_int32),
        ("timer_frames_per_level", C.c_int32),
        ("device", C.c_int32),
        ("map", C.c_char_p),
        ("map_portal", C.POINTER(C.c_int16)),
        ("player", Profile),
        ("npc", Profile),
        ("items", Items),
        ("n_agent_profiles", C.c_int32),
        ("agent_profile", Profile * MAX_AGENTS),
    ]


class ArenaHdr(C.Structure):
    _fields_ = [
        ("frame", C.c_int64), ("kills", C.c_int64), ("teams_kills", C.c_int64), ("loot", C.c_int64),
        ("chests", C.c_int64), ("jomle", C.c_int64), ("tb", C.c_int64), ("serial", C.c_int64),
        ("steps", C.c_int64), ("episodes", C.c_int64),
        ("rng", C.c_int32 * 18),
        ("done", C.c_int32), ("outcome", C.c_int32),
    ]


class HumanRec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("alive", "remote", "rnpc", "profile", "f", "r", "c", "way", "team", "hp", "stamina", "mindamage",
                 "kills", "damage", "effect", "vec", "ind")] + [
        ("cons", C.c_int32 * 4), ("throw_cnt", C.c_int32 * 4),
        ("blocks", C.c_int32), ("portals", C.c_int32), ("portal_ind", C.c_int32)]


class ZombieRec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("alive", "f", "r", "c", "hp", "mindamage", "super_")]


class BulletRec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("alive", "f", "r", "c", "way", "traveled", "damage", "effect", "range", "owner", "ref")]


class PortalRec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("active", "f", "r", "c")]


class ResetSel(C.Structure):
    """sf_reset_sel: which arenas sf_reset_arenas restarts, and on which seeds (device pointers as integers)."""
    _fields_ = [
        ("d_mask", C.c_void_p), ("mask_stride", C.c_int32), ("done_too", C.c_int32), ("max_steps", C.c_int32),
        ("d_tb", C.c_void_p), ("d_serial", C.c_void_p), ("d_selected", C.c_void_p),
    ]


SNAPSHOT_BLOB_HEADER = 24  # bytes in front of a slot's bytes in a blob: magic, layout version, payload length, fingerprint
SNAPSHOT_BLOB_MAGIC = 0x4E534653  # "SFSN", little-endian
SNAPSHOT_BLOB_VERSION = 1
SNAPSHOT_STATUS_WORDS = 4  # sf_snapshot_status: arenas skipped for an empty slot, for an index out of range, 0, 0
SNAPSHOT_EXPORTS = ("snapshot_create", "snapshot_destroy", "snapshot_slot_bytes", "snapshot_save", "snapshot_load",
                    "snapshot_status", "snapshot_export", "snapshot_import")


def bind_snapshot(lib, prefix):
    """Declare the sf_snapshot_* entry points (strikeforce.h) on a loaded library; handles and pointers as integers."""
    g = lambda n: getattr(lib, prefix + n)
    vp = C.c_void_p
    g("snapshot_create").argtypes = [vp, C.c_int32, C.POINTER(vp)]
    g("snapshot_destroy").argtypes = [vp]
    g("snapshot_slot_bytes").argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    g("snapshot_save").argtypes = [vp, vp, vp]
    g("snapshot_load").argtypes = [vp, vp, vp]
    g("snapshot_status").argtypes = [vp, C.POINTER(C.c_int32 * SNAPSHOT_STATUS_WORDS)]
    g("snapshot_export").argtypes = [vp, C.c_int32, vp, C.c_int64]
    g("snapshot_import").argtypes = [vp, C.c_int32, vp, C.c_int64]
    for n in SNAPSHOT_EXPORTS:
        g(n).restype = C.c_int
    return lib


VITALS_WORDS, DELTA_WORDS = 16, 8  # SF_VITALS_WORDS, SF_DELTA_WORDS
SIG_PRESENT, SIG_DIED, SIG_ENDED, SIG_REBASED, SIG_UNRESOLVED, SIG_IDLE = 1, 2, 4, 8, 16, 32  # SF_SIG_*
VITALS_FIELDS = ("flags", "hp", "stamina", "mindamage", "kills", "damage", "effect", "floor", "row", "col", "way", "team",
                 "arena_kills", "teams_kills", "loot", "steps")
DELTA_FIELDS = ("flags", "d_kills", "d_teams_kills", "d_loot", "d_damage", "d_effect", "d_hp", "outcome")
SIGNALS_STATUS_WORDS = 4  # sf_signals_status: records with UNRESOLVED, records rebased by the detection alone, 0, 0
SIGNALS_EXPORTS = ("signals_create", "signals_destroy", "signals_step", "signals_status")


class RewardWeights(C.Structure):
    """sf_reward_weights: per_step, w[6] over sf_results' words 0..5, died, outcome[8] by SF_* outcome code."""
    _fields_ = [("per_step", C.c_float), ("w", C.c_float * 6), ("died", C.c_float), ("outcome", C.c_float * 8)]


class SignalsIO(C.Structure):
    """sf_signals_io: the optional outputs and the rebase mask of one sf_signals_step (device pointers as integers)."""
    _fields_ = [("d_vitals", C.c_void_p), ("d_delta", C.c_void_p), ("d_reward", C.c_void_p), ("d_rebase", C.c_void_p),
                ("weights", RewardWeights)]


def bind_signals(lib, prefix):
    """Declare the sf_signals_* entry points (strikeforce.h) on a loaded library; handles and pointers as integers."""
    g = lambda n: getattr(lib, prefix + n)
    vp = C.c_void_p
    g("signals_create").argtypes = [vp, C.POINTER(vp)]
    g("signals_destroy").argtypes = [vp]
    g("signals_step").argtypes = [vp, vp, C.POINTER(SignalsIO)]
    g("signals_status").argtypes = [vp, C.POINTER(C.c_int64 * SIGNALS_STATUS_WORDS)]
    for n in SIGNALS_EXPORTS:
        g(n).restype = C.c_int
    return lib


N_COMMANDS = 30  # SF_N_COMMANDS; SF_COMMANDS is ALL_COMMANDS: bit k of an action-mask word stands for ALL_COMMANDS[k]
ACTION_MASK_EXPORTS = ("action_mask_device", "action_mask")


class ActionMaskIO(C.Structure):
    """sf_action_mask_io: the optional outputs of one sf_action_mask_device (device pointers as integers) and the host
    string of the action set d_actions is laid out by."""
    _fields_ = [("d_commands", C.c_void_p), ("action_string", C.c_char_p), ("d_actions", C.c_void_p)]


def bind_action_mask(lib, prefix):
    """Declare sf_action_mask_device / sf_action_mask (strikeforce.h) on a loaded library; handles and pointers as integers."""
    g = lambda n: getattr(lib, prefix + n)
    g("action_mask_device").argtypes = [C.c_void_p, C.POINTER(ActionMaskIO)]
    g("action_mask").argtypes = [C.c_void_p, C.c_void_p]
    for n in ACTION_MASK_EXPORTS:
        g(n).restype = C.c_int
    return lib


STATE_COUNT_WORDS = 8  # SF_STATE_COUNT_WORDS
STATE_COUNT_FIELDS = ("humans_alive", "zombies_alive", "bullets_alive", "portals_active",
                      "humans_extent", "zombies_extent", "bullets_extent", "portals_extent")
STATE_OUTPUTS = ("d_hdr", "d_humans", "d_zombies", "d_bullets", "d_portals", "d_cell_flags", "d_cell_dmg", "d_cell_portal",
                 "d_counts", "d_digest")  # the order of sf_state_bytes' ten sizes
STATE_EXPORTS = ("state_device", "state_bytes")


class StateIO(C.Structure):
    """sf_state_io: the id list, the cuts and the optional outputs of one sf_state_device (device pointers as integers)."""
    _fields_ = [("d_arena_ids", C.c_void_p), ("rows", C.c_int32),
                ("humans", C.c_int32), ("zombies", C.c_int32), ("bullets", C.c_int32), ("portals", C.c_int32)] + [
        (n, C.c_void_p) for n in STATE_OUTPUTS]


def bind_state(lib, prefix):
    """Declare sf_state_device / sf_state_bytes (strikeforce.h) on a loaded library; handles and pointers as integers."""
    g = lambda n: getattr(lib, prefix + n)
    g("state_device").argtypes = [C.c_void_p, C.POINTER(StateIO)]
    g("state_bytes").argtypes = [C.c_void_p, C.POINTER(StateIO), C.POINTER(C.c_int64 * 10)]
    for n in STATE_EXPORTS:
        g(n).restype = C.c_int
    return lib


PUT_BAD_HDR, PUT_BAD_HUMAN, PUT_BAD_ZOMBIE, PUT_BAD_BULLET, PUT_BAD_PORTAL, PUT_BAD_CELL, PUT_BAD_ROW = 1, 2, 4, 8, 16, 32, 64  # SF_PUT_BAD_*
STATE_PUT_PARTS = ("d_hdr", "d_humans", "d_zombies", "d_bullets", "d_portals", "d_cell_flags", "d_cell_dmg", "d_cell_portal")
STATE_PUT_STATUS_FIELDS = ("written", "refused", "row_out_of_range", "reserved")  # sf_state_put_status
STATE_PUT_EXPORTS = ("state_put_device", "state_put_status", "load_arena")


class StatePutIO(C.Structure):
    """sf_state_put_io: the row map, the cuts, the optional parts and the two optional outputs of one sf_state_put_device
    (device pointers as integers)."""
    _fields_ = [("d_row_of_arena", C.c_void_p), ("rows", C.c_int32),
                ("humans", C.c_int32), ("zombies", C.c_int32), ("bullets", C.c_int32), ("portals", C.c_int32)] + [
        (n, C.c_void_p) for n in STATE_PUT_PARTS] + [("d_status", C.c_void_p), ("d_selected", C.c_void_p)]


def bind_state_put(lib, prefix):
    """Declare sf_state_put_device / sf_state_put_status / sf_load_arena (strikeforce.h) on a loaded library."""
    g = lambda n: getattr(lib, prefix + n)
    vp = C.c_void_p
    g("state_put_device").argtypes = [vp, C.POINTER(StatePutIO)]
    g("state_put_status").argtypes = [vp, C.POINTER(C.c_int64 * 4)]
    g("load_arena").argtypes = [vp, C.c_int32] + [vp] * 8
    for n in STATE_PUT_EXPORTS:
        g(n).restype = C.c_int
    return lib


RECORD_GAME_WORDS, RECORD_COUNT_WORDS = 12, 6  # SF_RECORD_GAME_WORDS, SF_RECORD_COUNT_WORDS
RECORD_GAME_ENDED, RECORD_CUT, RECORD_OVERFLOW, RECORD_BROKEN = 1, 2, 3, 4  # SF_RECORD_*
RECORD_COUNT_FIELDS = ("games", "bytes", "games_pending", "bytes_pending", "games_lost", "bytes_substituted")
RECORD_EXPORTS = ("record_create", "record_destroy", "record_step", "record_flush", "record_collect_device", "record_collect")


def bind_record(lib, prefix):
    """Declare the sf_record_* entry points (strikeforce.h) on a loaded library; handles and pointers as integers."""
    g = lambda n: getattr(lib, prefix + n)
    vp = C.c_void_p
    g("record_create").argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(vp)]
    g("record_destroy").argtypes = [vp]
    g("record_step").argtypes = [vp, vp, vp]
    g("record_flush").argtypes = [vp, vp]
    g("record_collect_device").argtypes = [vp, vp, C.c_int64, vp, C.c_int32, vp]
    g("record_collect").argtypes = [vp, vp, C.c_int64, vp, C.c_int32, vp]
    for n in RECORD_EXPORTS:
        g(n).restype = C.c_int
    return lib


def record_fields(struct):
    """(name, first int32 word, words) of every field of a record structure, in layout order."""
    return [(n, getattr(struct, n).offset // 4, getattr(struct, n).size // 4) for n, _ in struct._fields_]


def struct_to_dict(s):
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        out[name] = list(v) if hasattr(v, "__len__") else v
    return out


def bind(lib, prefix):
    """Declare argtypes/restypes of the C-ABI on a loaded library (prefix 'sf_' or 'sfo_')."""
    g = lambda n: getattr(lib, prefix + n)
    vp = C.c_void_p
    g("reset").argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    g("step").argtypes = [vp, C.c_char_p]
    g("observe").argtypes = [vp, C.POINTER(C.c_float)]
    g("results").argtypes = [vp, C.POINTER(C.c_int32)]
    g("done").argtypes = [vp, C.POINTER(C.c_uint8)]
    g("state_digest").argtypes = [vp, C.POINTER(C.c_uint64)]
    g("dump_arena").argtypes = [vp, C.c_int32, C.POINTER(ArenaHdr), C.POINTER(HumanRec), C.POINTER(ZombieRec),
                                C.POINTER(BulletRec), C.POINTER(PortalRec), C.POINTER(C.c_uint8),
                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    g("step_begin").argtypes = [vp]
    g("step_end").argtypes = [vp, C.c_char_p]
    g("agent_alive").argtypes = [vp, C.POINTER(C.c_uint8)]
    # (the oracle keeps its own per-arena entry, sfo_phase_draws, with 64-bit counts; a library of an earlier round,
    # loaded for an A/B through SF_LIBRARY_PATH, lacks the entry)
    if prefix != "sfo_" and hasattr(lib, prefix + "phase_draws"):
        g("phase_draws").argtypes = [vp, C.POINTER(C.c_int32)]
        g("phase_draws").restype = C.c_int
    for n in ("reset", "step", "observe", "results", "done", "state_digest", "dump_arena", "step_begin", "step_end",
              "agent_alive"):
        g(n).restype = C.c_int
    g("destroy").argtypes = [vp]
    return lib
