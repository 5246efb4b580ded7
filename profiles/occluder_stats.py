#!/usr/bin/env python3
"""What the shadow rays' occluder table saves, from a counting build made beforehand with
  make variant NAME=occstats EXTRA_HIPFLAGS=-DPT_OCCLUDER_STATS
on big-scene 1920x1080x64: per light the shadow walks, those with a lane in the shadow, those with every lane in the shadow, and of
the last how many the table's candidate alone would have ended. The counting walk itself is unchanged.
usage (GPU box, repo root): python3 profiles/occluder_stats.py build/variants/occstats flat|hier

With a third argument `certain` the build is one of
  make variant NAME=occstats2 EXTRA_HIPFLAGS=-DPT_OCCLUDER_STATS=2
whose diag[6] and diag[7] count instead, per light in 21 bits each (so fewer than 2,097,152 walks per light: checked), what the certain-shadow test (pt_certain.h)
would settle: of the walks the candidate alone ends, those in which its inscribed ball settles every shaded lane; and of ALL fully blocked walks, those the dark-light
guard (a light the launch found enclosed in a node's ball, pt_certain.h 4.-8.) settles before anything is read for the light. A walk the guard would settle in which some
lane is NOT blocked would be a wrong skip: the build counts those apart, and this script fails unless there are none. The launch's per-light records are printed too.
The counting walk is unchanged there as well (flat only: the hierarchical semantics has no table)."""
import ctypes, os, shutil, sys, tempfile, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tmp = tempfile.mkdtemp()
shutil.copytree(os.path.join(ROOT, "portrayer_amd"), os.path.join(tmp, "portrayer_amd"), ignore=shutil.ignore_patterns("csrc", "host"))
shutil.copy(os.path.join(sys.argv[1], "libportrayer_hip.so"), os.path.join(tmp, "portrayer_amd", "libportrayer_hip.so"))
sys.path.insert(0, tmp)
sys.path.insert(1, os.path.join(ROOT, "tests"))
from portrayer_amd import _hip as H, host
from scene_dsl import ASSETS, default_background
mode = sys.argv[2]
sc = host.Scene.example("big-scene", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_HIER if mode == "hier" else H.TRAVERSE_FLAT)
w, h = 1920, 1080
_, _, st = r.render(sc.camera, w, h, default_background(w, h), samples=64, seed=0, sample_mode=H.SAMPLE_RNG, stats=True, want_linear=False)
dark_nodes = None
if len(sys.argv) > 3 and sys.argv[3] == "certain":
    info = (ctypes.c_uint64 * 2)()
    assert H.lib().pt_test_dark_lights(r.context, None, 0, info) == 0 and info[0] == 3 and info[1] == 8
    words = (ctypes.c_uint32 * 24)()
    assert H.lib().pt_test_dark_lights(r.context, words, 24, info) == 0
    dark_nodes = [int(words[8 * l + 4]) - 1 for l in range(3)]  # the flattened node the light is enclosed in; -1: none
r.close()
d = st["diag"]
lo = lambda x: x & 0xFFFFFFFF
hi = lambda x: x >> 32
out = {"mode": mode, "shadow_rays": st["shadow"], "n_inner": st["n_inner"], "primary": st["primary"], "lights": []}
for l in range(3):
    out["lights"].append({"walks": lo(d[2 * l]), "some_lane_occluded": hi(d[2 * l]), "all_occluded": lo(d[2 * l + 1]), "candidate_ends": hi(d[2 * l + 1])})
if len(sys.argv) > 3 and sys.argv[3] == "certain":
    for l in range(3):
        assert out["lights"][l]["walks"] < (1 << 21), "a 21-bit field would overflow"
        out["lights"][l]["candidate_ends_and_its_ball_settles"] = (d[6] >> (21 * l)) & 0x1FFFFF
        out["lights"][l]["dark_light_guard_settles"] = (d[7] >> (21 * l)) & 0x1FFFFF
        out["lights"][l]["enclosed_in_node"] = dark_nodes[l]
        assert out["lights"][l]["dark_light_guard_settles"] <= out["lights"][l]["all_occluded"]
        assert dark_nodes[l] >= 0 or out["lights"][l]["dark_light_guard_settles"] == 0
    out["settled_with_a_lane_unblocked"] = st["kd_plane_miss"]
    assert st["kd_plane_miss"] == 0, "the dark-light guard settled a walk in which some lane is not blocked"
else:
    out["walks_with_candidate"] = lo(d[6]); out["candidate_from_own_tile"] = hi(d[6]); out["candidate_blocked_a_lane"] = d[7]
print("OCCSTATS " + json.dumps(out), flush=True)
