#!/usr/bin/env python3
"""What the primary rays' per-pixel candidate lists do on big-scene 1920x1080x64, from a counting build made beforehand with
  make variant NAME=plstats EXTRA_HIPFLAGS="-DPT_PIXEL_LIST_STATS -DPT_PL_K=14u"
The counting kernel evaluates every item's list beside its unchanged walk (pt_render_simple.h) and counts: items with a record, background items (empty list,
nothing left out), items whose list was cut at the cap, items that would fall back to the walk, items in which the list's result differs from the walk's (must
be 0), leaf tests per lane by list and by the primary walk, and the histogram of list lengths. The cap (PORTRAYER_PIXEL_LIST_CAP) is varied to show what a
smaller K would cost (a cap above the build's K is refused; without -DPT_PL_K=14u the build has the shipped K = 6).
usage (GPU box, repo root): python3 profiles/pixel_list_stats.py build/variants/plstats [cap ...]"""
import json, os, shutil, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tmp = tempfile.mkdtemp()
shutil.copytree(os.path.join(ROOT, "portrayer_amd"), os.path.join(tmp, "portrayer_amd"), ignore=shutil.ignore_patterns("csrc", "host"))
shutil.copy(os.path.join(sys.argv[1], "libportrayer_hip.so"), os.path.join(tmp, "portrayer_amd", "libportrayer_hip.so"))
sys.path.insert(0, tmp)
sys.path.insert(1, os.path.join(ROOT, "tests"))
from portrayer_amd import _hip as H, host
from scene_dsl import ASSETS, default_background
caps = [int(c) for c in sys.argv[2:]] or [None]  # (none given: the build's own K)
sc = host.Scene.example("big-scene", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
w, h = 1920, 1080
F = (1 << 21) - 1
bins = ["0", "1", "2", "3", "4", "5", "6", "7", "8", "9-10", "11-13", "14"]
for cap in caps:
    if cap is not None:
        os.environ["PORTRAYER_PIXEL_LIST_CAP"] = str(cap)
    _, _, st = r.render(sc.camera, w, h, default_background(w, h), samples=64, seed=0, sample_mode=H.SAMPLE_RNG, stats=True, want_linear=False)
    d = st["diag"]
    items = d[0] & F
    assert 0 < items < (1 << 21), "a 21-bit field would overflow (or the build has no -DPT_PIXEL_LIST_STATS)"
    hist = {b: (d[4 + k // 3] >> (21 * (k % 3))) & F for k, b in enumerate(bins)}
    out = {"cap": cap, "items": items, "background_items": (d[0] >> 21) & F, "marked_take_the_walk": (d[0] >> 42) & F,
           "cut_at_cap": d[1] & F, "would_fall_back": (d[1] >> 21) & F, "items_where_list_and_walk_differ": (d[1] >> 42) & F,
           "leaf_tests_by_list": d[2], "leaf_tests_by_walk": d[3], "primary": st["primary"], "n_inner_all_rays": st["n_inner"],
           "length_histogram": hist}
    out["share_background"] = round(out["background_items"] / items, 4)
    out["share_cut"] = round(out["cut_at_cap"] / items, 4)
    out["share_fall_back"] = round(out["would_fall_back"] / items, 4)
    out["leaf_tests_per_item_lane_by_list"] = round(d[2] / st["primary"], 3)
    out["leaf_tests_per_item_lane_by_walk"] = round(d[3] / st["primary"], 3)
    print("PLSTATS " + json.dumps(out), flush=True)
r.close()
