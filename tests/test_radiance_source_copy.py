"""pt_radiance.h restates pt_light_position and pt_lane_advance of pt_shade.h (pt_source_light_position, pt_source_advance) because the render kernels' code
objects must not change. This test keeps the copy honest without a GPU: the originals' text, with the signature lines and the handful of places
that read the render's camera, pixel, sample index and background replaced by the source policy's calls, must be the copy's text line for line. An edit of one
of the two that is not made in the other fails here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "portrayer_amd", "csrc")

STREAM = ("const uint32_t sample = pt_lane_sample(a, L.item);\n"
          "{i}PT_LANE_XY(a, L, lx, ly);\n"
          "{i}uint64_t pixel = (uint64_t)ly * a.width + lx;\n")
STREAM_NEW = ("const uint32_t sample = src.sample(a, L);\n"
              "{i}uint64_t pixel = src.stream(a, L);\n")


def function_text(text, start):
    """From `start` (the first line of a definition at column 0) to its closing brace at column 0, inclusive."""
    i = text.index(start)
    j = text.index("\n}\n", i) + 3
    return text[i:j]


def swap(text, old, new, count=1):
    assert text.count(old) == count, "pt_shade.h no longer has %d x %r: update the copy in pt_radiance.h and this list together" % (count, old)
    return text.replace(old, new)


def test_the_copy_is_the_original_with_the_policy_calls_in_place():
    shade = open(os.path.join(CSRC, "pt_shade.h")).read()
    rad = open(os.path.join(CSRC, "pt_radiance.h")).read()

    light = function_text(shade, "PT_HD PtVec3 pt_light_position(")
    light = swap(light, "PT_HD PtVec3 pt_light_position(const PtRenderArgs& a, const PtLane& L, const double* light, uint32_t draw0, bool* is_area) {",
                 "PT_HD PtVec3 pt_source_light_position(const PtRenderArgs& a, const PtLane& L, const double* light, uint32_t draw0, bool* is_area, const SRC& src) {")
    light = swap(light, STREAM.format(i=" " * 4), STREAM_NEW.format(i=" " * 4))
    assert "template <class SRC>\n" + light in rad, "pt_source_light_position differs from pt_light_position by more than its source calls"

    adv = function_text(shade, "template <bool STATS, bool TEX, bool HIER = false, int PARK = 0, bool FORK = false>\nPT_ADVANCE_ATTR void pt_lane_advance(")
    adv = swap(adv, "template <bool STATS, bool TEX, bool HIER = false, int PARK = 0, bool FORK = false>\n"
                    "PT_ADVANCE_ATTR void pt_lane_advance(const PtRenderArgs& a, PtLane& L, const PtHit& hit, const PtFrameRef& fr, PtCounters* cnt, uint32_t pre = 0) {\n",
               "template <bool TEX, bool HIER, int PARK, class SRC>\n"
               "PT_HD void pt_source_advance(const PtRenderArgs& a, PtLane& L, const PtHit& hit, const PtFrameRef& fr, PtCounters* cnt, uint32_t pre, const SRC& src) {\n"
               "    constexpr bool STATS = false, FORK = false;  // no counting variant, no fork / join: those branches of the render's text compile out\n")
    adv = swap(adv, "            double jx = 0.5, jy = 0.5;\n"
                    "            PT_LANE_XY(a, L, lx, ly);\n"
                    "            if (a.jitter_mode == PT_JITTER_RNG) {  // render.rs:38-39: x drawn before y\n"
                    "                const uint32_t sample = pt_lane_sample(a, L.item);\n"
                    "                uint64_t pixel = (uint64_t)ly * a.width + lx;\n"
                    "                jx = pt_rng_f64(a.seed, pixel, sample, 0);\n"
                    "                jy = pt_rng_f64(a.seed, pixel, sample, 1);\n"
                    "            }\n"
                    "            L.draw = 2;\n"
                    "            L.ray = pt_camera_ray(a.cam, (double)lx + jx, (double)ly + jy);\n",
               "            L.ray = src.primary(a, L);\n"
               "            L.draw = 2;  // draws 0 and 1 are the render's jitter, whatever the source\n")
    adv = swap(adv, "if (hit.node == PT_NO_HIT) { PT_LANE_XY(a, L, lx, ly); value = pt_background(a, lx, ly); returning = true; continue; }",
               "if (hit.node == PT_NO_HIT) { value = src.background(a, L); returning = true; continue; }")
    adv = swap(adv, "pt_light_position(a, L, light, L.draw, &is_area);", "pt_source_light_position(a, L, light, L.draw, &is_area, src);")
    adv = swap(adv, "pt_light_position(a, L, light, draw, &is_area);", "pt_source_light_position(a, L, light, draw, &is_area, src);")
    adv = swap(adv, STREAM.format(i=" " * 16), STREAM_NEW.format(i=" " * 16))
    adv = swap(adv, "                PT_LANE_XY(a, L, lx, ly);\n                PtVec3 bg = pt_background(a, lx, ly);\n", "                PtVec3 bg = src.background(a, L);\n")
    for leftover in ("pt_lane_sample", "PT_LANE_XY", "pt_background", "pt_camera_ray", "a.cam", "a.width", "a.jitter_mode"):
        assert leftover not in adv and leftover not in light, "the render's %s is still read where the source policy should be asked" % leftover
    assert adv in rad, "pt_source_advance differs from pt_lane_advance by more than its source calls"
    # and the copies are what the kernel calls
    assert re.search(r"pt_source_advance<TEX, HIER, PARK, PtRaySource>\(a, L, hit, fr, &cnt, 0u, src\)", rad) and "pt_lane_advance<" not in rad
