"""Which buffer comes back in which array, for every host form of the passes: ao, gather and direct at the caller's points, under a camera's pixels and at a
chart's texels; probe; rays with and without t_max; aov, guides, chart and radiance. Each form stages its buffers through the same scratch slots and PtBufs
whatever is asked for, so a call that asks for some of its buffers must give those the bits of the call that asks for all of them - in fresh arrays and in the
caller's own (`into`, prefilled with a sentinel) - and a call at a small size behind one at a larger size must give the bits it gave before the scratch grew.

The shapes are the smallest that cross a boundary where a slot or a size mix-up would show: 70 points (a wavefront of 64 and a partial one; at samples=4 the
point-major ambient-occlusion layout ends in a partial work item), 9 x 8 images and charts (an 8 x 8 tile and a partial one), 3 probes at 64 samples (the kernel
stores) and at 128 (the fold does); one scene with a mesh node, a point light and an area light; the flat and the k-d traversal."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the product's library is loaded: the process then has one HIP runtime, torch's)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from chart_restate import same_bits  # noqa: E402
from scene_dsl import Camera, Light, Mesh, Node  # noqa: E402
from test_gpu_chart import RED, cube_mesh, mesh_nodes, traverse_of, under_a_group  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ["flat", "kd"]
SMALL, LARGE = {"points": 70, "image": (9, 8), "probes": 3}, {"points": 200, "image": (20, 17), "probes": 7}
BG = (0.25, 0.5, 1.0)
CAMERA = Camera(eye=(0.6, 1.0, 4.5), center=(0.2, -0.3, 0.3))
LIGHTS = [Light(position=(3.0, 4.0, 9.0), color=(0.9, 0.9, 0.9)), Light(position=(-2.0, 5.0, 3.0), color=(0.5, 0.4, 0.3), area_a=(0.0, 0.5, 0.0), area_b=(0.5, 0.0, 0.0))]
KW = dict(samples=4, bias=1e-3, seed=5, pass_index=1)


class Ctx:
    """a renderer of the scene in one traversal and what the forms are called with: the mesh node and its unwrap, the camera, 340 surface points (a 20 x 17
    chart's texels, the unowned ones - invalid points, rays that are not traced - among them) and the rays cast back at them"""

    def __init__(self, host, H, mode):
        self.H = H
        hs = host_glue.host_scene(under_a_group([Node.geo(Mesh(cube_mesh(), True), RED)], lights=LIGHTS))
        self.r = host.Renderer(hs, traverse_of(H, mode))
        self.node, self.uv, self.cam = mesh_nodes(hs)[0], cube_mesh().tex_coords, host_glue.cam10(CAMERA)
        ch = self.r.chart(self.node, 20, 17, self.uv, want=("position", "normal"))
        deal = (np.arange(340) * 47) % 340  # (texels from all over the map among the first few)
        self.P, self.N = ch["position"].reshape(-1, 3)[deal], ch["normal"].reshape(-1, 3)[deal]
        self.O, self.D = self.P + 0.5 * self.N, -self.N
        self.t_max = np.where(np.arange(len(self.P)) % 3 == 0, 0.25, 0.75)  # (a third of the segments end in front of the surface)


def _points(c, size):
    n = size["points"]
    return c.P[:n], c.N[:n]


def _rays(c, size):
    n = size["points"]
    return c.O[:n], c.D[:n]


def _radiance(c, size, want, into):
    return c.r.radiance(*_rays(c, size), BG, seed=5, sample=1, into=None if into is None else into["rgb"])


# form -> (its table of buffers, the call: (context, size, want, into) -> the method's dict)
FORMS = {
    "ao": ("AO_BUFFERS", lambda c, s, want, into: c.r.ao(*_points(c, s), radius=3.0, want=want, into=into, **KW)),
    "ao_camera": ("AO_BUFFERS", lambda c, s, want, into: c.r.ao_camera(c.cam, *s["image"], radius=3.0, want=want, into=into, **KW)),
    "ao_chart": ("AO_BUFFERS", lambda c, s, want, into: c.r.ao_chart(c.node, *s["image"], c.uv, radius=3.0, want=want, into=into, **KW)),
    "gather": ("GATHER_BUFFERS", lambda c, s, want, into: c.r.gather(*_points(c, s), BG, want=want, into=into, **KW)),
    "gather_camera": ("GATHER_BUFFERS", lambda c, s, want, into: c.r.gather_camera(c.cam, *s["image"], BG, want=want, into=into, **KW)),
    "gather_chart": ("GATHER_BUFFERS", lambda c, s, want, into: c.r.gather_chart(c.node, *s["image"], BG, c.uv, want=want, into=into, **KW)),
    "direct": ("DIRECT_BUFFERS", lambda c, s, want, into: c.r.direct(*_points(c, s), to_light=True, want=want, into=into, **KW)),
    "direct_camera": ("DIRECT_BUFFERS", lambda c, s, want, into: c.r.direct_camera(c.cam, *s["image"], to_light=True, want=want, into=into, **KW)),
    "direct_chart": ("DIRECT_BUFFERS", lambda c, s, want, into: c.r.direct_chart(c.node, *s["image"], c.uv, to_light=True, want=want, into=into, **KW)),
    "probe_64": ("PROBE_BUFFERS", lambda c, s, want, into: c.r.probe(c.O[:s["probes"]], BG, samples=64, seed=5, pass_index=1, want=want, into=into)),
    "probe_128": ("PROBE_BUFFERS", lambda c, s, want, into: c.r.probe(c.O[:s["probes"]], BG, samples=128, seed=5, pass_index=1, want=want, into=into)),
    "rays": ("RAYS_BUFFERS", lambda c, s, want, into: c.r.rays(*_rays(c, s), want=want, into=into)),
    "rays_t_max": ("RAYS_BUFFERS", lambda c, s, want, into: c.r.rays(*_rays(c, s), want=want, into=into, t_max=c.t_max[:s["points"]])),
    "aov": ("AOV_BUFFERS", lambda c, s, want, into: c.r.aov(c.cam, *s["image"], want=want, into=into)),
    "guides": ("GUIDES_BUFFERS", lambda c, s, want, into: c.r.guides(c.cam, *s["image"], want=want, into=into)),
    "chart": ("CHART_BUFFERS", lambda c, s, want, into: c.r.chart(c.node, *s["image"], c.uv, want=want, into=into)),
    "radiance": ({"rgb": (np.float64, 3)}, _radiance),
}
# what tells a form's buffers apart: were these all zero, a mix-up among them could not show
ALIVE = {"ao": ("occluded", "valid", "bent"), "gather": ("sum", "valid"), "direct": ("sum", "lit", "valid"), "probe": ("sh", "valid"), "rays": ("position", "occluded"),
         "aov": ("position", "normal"), "guides": ("albedo", "normal"), "chart": ("position", "covered"), "radiance": ("rgb",)}


@pytest.fixture(scope="module")
def contexts():
    from portrayer_amd import _hip as H
    from portrayer_amd import host
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = Ctx(host, H, mode)
        return made[mode]

    yield get
    for c in made.values():
        c.r.close()


def sentinel_like(a):
    s = np.empty_like(a)
    s.view(np.uint8)[...] = 0xA5
    return s


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("mode", MODES)
def test_some_of_a_forms_buffers_are_the_bits_of_all_of_them_also_behind_a_larger_call(contexts, mode, form):
    c = contexts(mode)
    table, call = FORMS[form]
    names = tuple(getattr(c.H, table) if isinstance(table, str) else table)
    full = call(c, SMALL, names, None)
    for name in ALIVE[form.split("_")[0]]:
        assert np.any(full[name]), "%s: %s is all zero, the shapes prove nothing" % (form, name)
    subsets = [w for k in range(1, len(names)) for w in itertools.combinations(names, k)]
    for want in subsets + [names]:
        where = "%s %s want=%r" % (form, mode, want)
        if want != names:
            got = call(c, SMALL, want, None)
            assert [n for n in names if n in got] == list(want), where
            for name in want:
                assert same_bits(got[name], full[name]), "%s: %s in a fresh array" % (where, name)
        into = {name: sentinel_like(full[name]) for name in want}
        got = call(c, SMALL, want, into)
        assert [n for n in names if n in got] == list(want), where
        for name in want:
            assert got[name] is into[name] and same_bits(into[name], full[name]), "%s: %s through into" % (where, name)
    larger = call(c, LARGE, names, None)
    again = call(c, SMALL, names, None)
    for name in names:
        assert larger[name].shape != full[name].shape
        assert same_bits(again[name], full[name]), "%s %s: %s behind a larger call" % (form, mode, name)
    one = call(c, SMALL, names[-1:], None)
    assert same_bits(one[names[-1]], full[names[-1]]), "%s %s: %s alone behind a larger call" % (form, mode, names[-1])
