"""What a render launch has and where it lies (pt_plan_launch, csrc/pt_api.hip; PtLaunchPlan, csrc/pt_context.h), asked of pt_test_launch_plan - no context, no
device - for a table of a few hundred launches: the scenes of tests/golden/kernel_choice/ (their traits, whether they are textured), each with a mode, counting or plain,
a number of lights, of pixel slots, of nodes, a lane layout and a resident grid drawn from the axes below, under no switch and under each switch the planner
reads at its off value and at its boundary values.

The rules are restated here from the comments of the planner and of the kernels that rely on them (pt_render_simple.h), not recorded from the planner: `expected`."""
import ctypes as C
import json
import os
import random

import pytest

from scene_dsl import GOLDEN

TABLE = os.path.join(GOLDEN, "kernel_choice", "table.json")
TRAITS = ("traverse", "n_nodes", "n_lights", "has_meshes", "has_kdmesh", "instanced_tris", "reflective", "reflective_opaque", "glossy", "area_light")
FLAT_NOMESH, HIER_NOMESH = 3, 6                    # include/portrayer_hip.h: PT_KERNEL_MODE_*
BLOCK, PL_MAX_NODES, PL_K, PL_PENDING, PL_WORDS, DARK_WORDS, FINE_QUEUES, BATCH_MAX = 256, 65536, 6, 1024, 8, 8, 64, 8  # pt_trace.h, pt_pixel_list.h, pt_certain.h, pt_shade.h
OCC_LIMIT = 4 << 20
SWITCH_NAMES = ("PORTRAYER_SHADOW_CACHE", "PORTRAYER_DARK_LIGHTS", "PORTRAYER_PIXEL_LISTS", "PORTRAYER_BACKGROUND_SKIP", "PORTRAYER_PIXEL_LIST_CAP", "PORTRAYER_PIXEL_LIST_PENDING",
                "PORTRAYER_FINE_QUEUES", "PORTRAYER_BATCH_MAX", "PORTRAYER_OCC_SEED", "PORTRAYER_ITEM_STRIDE", "PORTRAYER_NO_TEX", "PORTRAYER_WAVES", "PORTRAYER_KD_WAVES",
                "PORTRAYER_CHAIN", "PORTRAYER_CHAIN_WAVES", "PORTRAYER_PARK", "PORTRAYER_FORK", "PORTRAYER_LDS_BUDGET_KB", "PORTRAYER_LDS_STACK")
# each switch of the planner at its off value and at its boundary values (the kernel's own switches: tests/test_kernel_choice.py)
SWITCHES = ["", "PORTRAYER_SHADOW_CACHE=0", "PORTRAYER_SHADOW_CACHE=1", "PORTRAYER_DARK_LIGHTS=0", "PORTRAYER_DARK_LIGHTS=1", "PORTRAYER_PIXEL_LISTS=0", "PORTRAYER_PIXEL_LISTS=1",
            "PORTRAYER_BACKGROUND_SKIP=0", "PORTRAYER_BACKGROUND_SKIP=1", "PORTRAYER_PIXEL_LIST_CAP=0", "PORTRAYER_PIXEL_LIST_CAP=6", "PORTRAYER_PIXEL_LIST_PENDING=1",
            "PORTRAYER_PIXEL_LIST_PENDING=1024", "PORTRAYER_FINE_QUEUES=0", "PORTRAYER_FINE_QUEUES=64", "PORTRAYER_FINE_QUEUES=65", "PORTRAYER_FINE_QUEUES=-1", "PORTRAYER_BATCH_MAX=1",
            "PORTRAYER_BATCH_MAX=0", "PORTRAYER_BATCH_MAX=32", "PORTRAYER_OCC_SEED=7", "PORTRAYER_OCC_SEED=all:0", "PORTRAYER_OCC_SEED=", "PORTRAYER_ITEM_STRIDE=golden",
            "PORTRAYER_PARK=0", "PORTRAYER_WAVES=5"]
MALFORMED = [("PORTRAYER_OCC_SEED=12x", "PORTRAYER_OCC_SEED=12x: expected all:<node> or a decimal seed"), ("PORTRAYER_OCC_SEED=all:", None), ("PORTRAYER_OCC_SEED=all:x", None),
             ("PORTRAYER_OCC_SEED=all:255", "PORTRAYER_OCC_SEED=all:255: K must be a node index below 255"),
             ("PORTRAYER_PIXEL_LIST_CAP=7", "PORTRAYER_PIXEL_LIST_CAP=7: expected 0 .. 6"), ("PORTRAYER_PIXEL_LIST_CAP=-1", None), ("PORTRAYER_PIXEL_LIST_CAP=2x", None),
             ("PORTRAYER_PIXEL_LIST_PENDING=0", "PORTRAYER_PIXEL_LIST_PENDING=0: expected 1 .. 1024"), ("PORTRAYER_PIXEL_LIST_PENDING=1025", "PORTRAYER_PIXEL_LIST_PENDING=1025: expected 1 .. 1024"),
             ("PORTRAYER_PIXEL_LIST_PENDING=many", None)]


def work_shape(width, height, samples):
    """pt_fill_work restated for a whole-image slice on one rank: how a launch's 64-lane wavefronts are laid over pixels x chunks x samples."""
    tiles_x, tiles_y = (width + 7) // 8, (height + 7) // 8
    n_slots = tiles_x * tiles_y * 64
    n_chunks = (samples + 7) // 8
    k = 8
    if samples < 8:
        k = 1
        while k < samples:
            k *= 2
    cc = 1
    if k == 8:
        for cand in (8, 4, 2):
            slots = (n_chunks + cand - 1) // cand * cand
            if (slots - n_chunks) * 16 <= n_chunks:
                cc = cand
                break
    n_items = (n_slots // 64) * ((n_chunks + cc - 1) // cc) * (k * cc)
    return dict(n_slots=n_slots, n_items=n_items, n_chunks=n_chunks, k_log2=k.bit_length() - 1, c_log2=cc.bit_length() - 1, tiles_x=tiles_x, tile_ranks=1)


def plan_of(H, traits, stats=False, mode=-1, textured=False, n_nodes=None, n_lights=None, stack_cap=24, grid=768, expect=0, **shape):
    """pt_test_launch_plan for a scene of these traits: the plan's words as a list of ints - or, where `expect` is an error code, the words of the refusal."""
    q = H.PtLaunchQuery(traits=H.PtSceneTraits(**traits), mode=mode, textured=int(textured), stats=int(stats),
                        n_nodes=traits["n_nodes"] if n_nodes is None else n_nodes, n_lights=traits["n_lights"] if n_lights is None else n_lights,
                        stack_cap=stack_cap, grid=grid, **shape)
    words, err = (C.c_uint64 * H.PLAN_WORDS)(), C.create_string_buffer(256)
    rc = H.lib().pt_test_launch_plan(C.byref(q), words, err, len(err))
    assert rc == expect, (rc, err.value.decode(), traits, shape)
    return err.value.decode() if expect else [int(w) for w in words]


def slots_at_the_limit(n_lights):
    """The pixel slots whose occluder table (a word per 8x8 tile and light) is the largest of at most 4 MB, and the next launch up."""
    tiles = OCC_LIMIT // (4 * n_lights)
    return [tiles * 64, (tiles + 1) * 64]


def rows():
    """-> dicts: the query's fields. `traits` and `textured` from the golden table's scenes, two rows a scene; the rest drawn from the axes by a seeded generator (the same
    table in every run), the mesh-free flat mode - the one that has everything - for half of the rows whatever the scene."""
    with open(TABLE) as fh:
        t = json.load(fh)
    assert tuple(t["traits"]) == TRAITS
    rng = random.Random(18)
    out = []
    for k, sc in enumerate(t["scenes"] + t["scenes"]):
        traits = dict(zip(TRAITS, sc["traits"]))
        n_lights = rng.choice((0, 1, 32, 33))
        n_slots = rng.choice((0, 64, 4096, "under", "over", 64, 4096))
        if n_slots in ("under", "over"):
            n_slots = slots_at_the_limit(max(n_lights, 1))[n_slots == "over"]
        k_log2, c_log2 = rng.choice(((3, 3), (3, 2), (3, 3)))
        n_chunks = rng.choice((1, 8, 13, 700))
        mode = rng.choice((FLAT_NOMESH,) * 10 + (-1, -1) + tuple(range(1, 10)))
        traits["n_lights"] = n_lights
        groups = (n_chunks + (1 << c_log2) - 1) >> c_log2
        out.append(dict(traits=traits, textured=bool(sc["textured"]), mode=mode, stats=rng.random() < 0.4, n_nodes=rng.choice((0, 1, PL_MAX_NODES, PL_MAX_NODES + 1, 255)),
                        n_lights=n_lights, stack_cap=rng.randrange(8, 100), n_slots=n_slots, n_items=(n_slots // 64) * groups * (1 << (k_log2 + c_log2)), n_chunks=n_chunks,
                        k_log2=k_log2, c_log2=c_log2, tiles_x=rng.randrange(1, 8), tile_ranks=rng.randrange(1, 4), grid=rng.choice((1, 768))))
    return out


def expected(H, row, env, variant):
    """The rules, from the comments: what a launch of `row` under the switches `env` has. variant: its kernel (pt_stats.kernel_variant)."""
    on = lambda name: int(env.get(name, "1") or "0") > 0
    mode = row["mode"]
    tiles, flat = row["n_slots"] // 64, mode == FLAT_NOMESH
    # the occluder table: the two mesh-free modes that are not k-d, one word per own tile and light, left out above 4 MB and by PORTRAYER_SHADOW_CACHE=0
    occ_bytes = tiles * row["n_lights"] * 4
    occluders = mode in (FLAT_NOMESH, HIER_NOMESH) and 0 < occ_bytes <= OCC_LIMIT and on("PORTRAYER_SHADOW_CACHE")
    # pt_render_simple.h: "a launch of this mode that has an occluder table has the certain-shadow table" - a table is per node: none without nodes
    certain = flat and row["n_nodes"] > 0 and occluders
    # the dark-light records lie in front of the occluder table of the flat launches; the kernel that fills them reads the certain-shadow table
    dark_records = flat and occluders
    dark_lights = dark_records and certain and on("PORTRAYER_DARK_LIGHTS")
    # "every launch in that mode gets an eye table whichever kernel runs", and the list header with it
    eye = flat and row["n_nodes"] > 0
    line = not variant & (H.KERNEL_INTERPRETER | H.KERNEL_CHAIN)
    # the lists: a kernel that reads them (plain, straight-line), one pixel per wavefront, node indices of 16 bits, some pixel, and the switch
    lists = eye and not row["stats"] and line and row["k_log2"] + row["c_log2"] == 6 and row["n_nodes"] <= PL_MAX_NODES and row["n_slots"] > 0 and on("PORTRAYER_PIXEL_LISTS")
    queue = lists and on("PORTRAYER_BACKGROUND_SKIP")
    has = (occluders * H.PLAN_HAS_OCCLUDERS | eye * H.PLAN_HAS_EYE_TABLE | certain * H.PLAN_HAS_CERTAIN_TABLE | dark_records * H.PLAN_HAS_DARK_RECORDS |
           dark_lights * H.PLAN_HAS_DARK_LIGHTS | eye * H.PLAN_HAS_LIST_HEADER | lists * H.PLAN_HAS_PIXEL_LISTS | queue * H.PLAN_HAS_QUEUE)
    # one item at a time from 16 queues for scenes whose hits spawn rays and for launches of at most 2048 items per resident wavefront, else batches
    fine = 16 if row["traits"]["reflective"] or row["n_items"] <= 2048 * max(row["grid"] * (BLOCK // 64), 1) else 0
    if "PORTRAYER_FINE_QUEUES" in env:
        fine = max(0, min(FINE_QUEUES, int(env["PORTRAYER_FINE_QUEUES"])))
    batch = max(1, int(env["PORTRAYER_BATCH_MAX"])) if "PORTRAYER_BATCH_MAX" in env else BATCH_MAX
    return dict(has=has, occ_bytes=occ_bytes if occluders else 0, dark_bytes=row["n_lights"] * DARK_WORDS * 4 if dark_records else 0, fine_queues=fine, batch_max=batch,
                list_cap=int(env.get("PORTRAYER_PIXEL_LIST_CAP", PL_K)), list_pending=int(env.get("PORTRAYER_PIXEL_LIST_PENDING", PL_PENDING)))


def check_row(H, row, env, misc_head):
    w = plan_of(H, **row)
    P = lambda name: w[getattr(H, "PLAN_" + name)]
    # the kernel: pt_test_kernel_choice's for the same traits
    mode, variant = C.c_uint32(), C.c_uint32()
    t = H.PtSceneTraits(**row["traits"])
    choice = H.lib().pt_test_kernel_choice
    choice.restype, choice.argtypes = C.c_int, [C.POINTER(H.PtSceneTraits), C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    assert choice(C.byref(t), row["mode"], int(row["textured"]), C.byref(mode), C.byref(variant)) == 0
    assert (P("KERNEL_MODE"), P("KERNEL_VARIANT")) == (mode.value, variant.value | (H.KERNEL_COUNTING if row["stats"] else 0)), row
    assert P("MORE_WAVES") in (0, 4, 5, 6) and (P("MORE_WAVES") or 3) == variant.value & H.KERNEL_WAVES_MASK, row
    want = expected(H, dict(row, mode=mode.value), env, variant.value)
    has = P("HAS")
    assert has == want["has"], (row, env, has, want["has"])
    for name in ("occ_bytes", "dark_bytes", "fine_queues", "batch_max", "list_cap", "list_pending"):
        assert P(name.upper()) == want[name], (name, row, env)
    # the coupled rules once more, on the plan's own words
    assert not has & H.PLAN_HAS_CERTAIN_TABLE or has & H.PLAN_HAS_OCCLUDERS
    assert not has & H.PLAN_HAS_DARK_LIGHTS or has & H.PLAN_HAS_CERTAIN_TABLE
    assert not has & H.PLAN_HAS_PIXEL_LISTS or has & H.PLAN_HAS_EYE_TABLE
    assert not has & H.PLAN_HAS_QUEUE or (has & H.PLAN_HAS_PIXEL_LISTS and P("ITEM_STRIDE") == 1), (row, env)
    # how the work is dealt
    assert P("N_LANES") == row["grid"] * BLOCK and P("WORK_DIV") == row["grid"] * (BLOCK // 64) * 8 and P("GRID_SHARE") == 1
    assert 1 <= P("ITEM_STRIDE") < max(row["n_items"], 2)
    assert P("OCC_ROW") == max(row["tiles_x"] // row["tile_ranks"], 1)
    assert 2 <= P("STACK_LDS_CAP") and P("ACCUM_BYTES") == row["n_slots"] * row["n_chunks"] * 24
    assert P("SPILL_BYTES") == (16 if not P("NEEDS_SPILL") else P("N_LANES") * 11 * 16 * 8) and P("NEEDS_SPILL") == int(bool(row["traits"]["reflective"] or row["traits"]["n_lights"] > 32))
    assert P("STACK_SPILL_BYTES") >= P("N_LANES") * row["stack_cap"] * 4
    # `misc`: head (the same in every launch), dark-light records, occluder table - in that order, nothing between them, words
    assert P("DARK_OFF") == misc_head and misc_head % 8 == 0 and misc_head >= 256 + 8
    assert P("OCC_OFF") == P("DARK_OFF") + P("DARK_BYTES") and P("MISC_BYTES") == P("OCC_OFF") + P("OCC_BYTES")
    assert P("DARK_OFF") % 4 == 0 and P("OCC_OFF") % 4 == 0
    # `eye_tab`: eye table (12 doubles a node), certain-shadow table (4 floats a node), header (64 bytes on a 64-byte boundary), records, queue and tile masks
    n, slots = row["n_nodes"], row["n_slots"]
    assert P("CERTAIN_OFF") == 96 * n and P("CERTAIN_OFF") % 8 == 0
    if has & H.PLAN_HAS_LIST_HEADER:
        assert 112 * n <= P("HEADER_OFF") < 112 * n + 64 and P("HEADER_OFF") % 64 == 0 and P("RECORDS_OFF") == P("HEADER_OFF") + 64
    else:
        assert P("HEADER_OFF") == P("RECORDS_OFF") == 112 * n
    assert P("QUEUE_OFF") == P("RECORDS_OFF") + (slots * PL_WORDS * 4 if has & H.PLAN_HAS_PIXEL_LISTS else 0)
    end = P("QUEUE_OFF") + (slots * 4 + (slots // 64) * 8 if has & H.PLAN_HAS_QUEUE else 0)
    assert P("QUEUE_OFF") % 8 == 0  # (the tile masks behind the ids are 64-bit words: slots x 4 is a multiple of 8)
    assert P("EYE_TAB_BYTES") == (end if has & (H.PLAN_HAS_EYE_TABLE | H.PLAN_HAS_CERTAIN_TABLE) else 0), (row, env)
    assert P("HEADER_FILL") == 0
    # PORTRAYER_OCC_SEED asks only where there is a table to seed
    seed = env.get("PORTRAYER_OCC_SEED", "")
    kind = 0 if not (seed and has & H.PLAN_HAS_OCCLUDERS) else (2 if seed.startswith("all:") else 1)
    assert P("OCC_SEED") == kind and (kind == 0 or P("OCC_SEED_VALUE") == int(seed.split(":")[-1])), (row, env)
    return has


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def set_switches(monkeypatch, switch):
    for k in SWITCH_NAMES:
        monkeypatch.delenv(k, raising=False)
    env = dict(kv.split("=") for kv in switch.split())
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return env


def test_the_table_covers_the_axes():
    table = rows()
    assert len(table) >= 200
    assert {r["mode"] for r in table} >= set(range(1, 10)) | {-1}
    flat = [r for r in table if r["mode"] == FLAT_NOMESH]
    for key, values in (("n_lights", (0, 1, 32, 33)), ("n_nodes", (0, 1, PL_MAX_NODES, PL_MAX_NODES + 1)), ("grid", (1, 768)), ("stats", (False, True)), ("textured", (False, True))):
        assert {r[key] for r in flat} >= set(values), key
    assert {r["k_log2"] + r["c_log2"] for r in flat} == {5, 6}
    assert {0, 64, 4096} <= {r["n_slots"] for r in flat}
    for n_lights in (1, 32, 33):  # a table of exactly 4 MB or just under it, and the next launch up
        under, over = slots_at_the_limit(n_lights)
        assert under // 64 * n_lights * 4 <= OCC_LIMIT < over // 64 * n_lights * 4
        assert any(r["n_slots"] == under and r["n_lights"] == n_lights for r in table) and any(r["n_slots"] == over and r["n_lights"] == n_lights for r in table), n_lights
    assert any(r["n_items"] > 2048 * r["grid"] * 4 for r in table) and any(0 < r["n_items"] <= 2048 * r["grid"] * 4 for r in table)


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: s or "default")
def test_every_row_is_laid_out_by_the_rules(H, monkeypatch, switch):
    env = set_switches(monkeypatch, switch)
    table = rows()
    misc_head = plan_of(H, **table[0])[H.PLAN_DARK_OFF]
    seen = 0
    for row in table:
        if env.get("PORTRAYER_OCC_SEED", "").startswith("all:") and row["n_nodes"] == 0:
            continue  # (no node to name: refused, test_a_malformed_switch_is_refused)
        seen |= check_row(H, row, env, misc_head)
    if switch == "":
        assert seen == 255  # every table and list is had by some row
        limits = [r for r in table if r["mode"] == FLAT_NOMESH and r["n_slots"] > 4096]
        assert {bool(plan_of(H, **r)[H.PLAN_OCC_BYTES]) for r in limits} == {False, True}


@pytest.mark.parametrize("switch,words", MALFORMED)
def test_a_malformed_switch_is_refused(H, monkeypatch, switch, words):
    set_switches(monkeypatch, switch)
    traits = dict(zip(TRAITS, [1, 255, 1, 0, 0, 0, 0, 1, 0, 0]))  # 255 spheres, one light, flat_scene: a launch with every table
    got = plan_of(H, traits, expect=H.ERR_ARGUMENT, **work_shape(16, 16, 64))
    assert got.startswith(switch.replace("=", "=", 1) + ": ") and (words is None or got == words), got
    if "OCC_SEED" in switch:  # no table to seed (the k-d semantics): the switch is not read
        assert plan_of(H, dict(traits, traverse=2), **work_shape(16, 16, 64))[H.PLAN_OCC_SEED] == 0
