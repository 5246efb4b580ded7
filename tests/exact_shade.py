"""The reference's shading restated in multi-precision arithmetic, on top of exact_ref's cast() (test infrastructure).

Written from material.rs, light.rs and ray.rs:139-148 only, not from oracle/ or the kernels: Ray::color and Material::hit_color expression by expression,
including what a port gets plausibly wrong (a shadow ray's range has no end, `view` and the reflected and refracted directions keep the caller's direction
length, the normal is never turned towards the viewer, `specular > EPSILON`, the exponent 4 * shininess, `cos_incident` from the REFRACTED direction on
leaving, powi(5), the background at depth 11, the glossy basis' two offset vectors, the quadratic falloff, area coordinates 2u - 1). Hit points and
secondary directions go to the next cast unrounded. pow is mp.power; powi(5) is four multiplications.

thread_rng cannot be restated: `draws` is a callable that yields the next number of the ray's stream in the project's own draw order (DESIGN 2 "Sampling":
two per area light in light order, two for a glossy material, then the reflected subtree, then the refracted one).

Every comparison in the ray tree records a margin as exact_ref.Trace does: every cast's own margins (the shadow casts' too), `under_sqrt < 0`,
`ray_dir.dot(normal) < 0` and the glossy `abs() < EPSILON` tests. A division by a zero light distance, the expect() that would panic
(material.rs:257-258), a NaN and a k-d panic are margin 0. The ray's margin is the smallest of its tree; below 2^-30 the ray is fragile.

Out of scope: textures, normal maps, uv_trans and KDMesh.
"""
from __future__ import annotations

import math
from collections import deque

from mpmath import mp, mpf

import exact_ref
from exact_ref import EPS_F64, FRAGILE, PREC, _cross, _dot, _margin  # noqa: F401

# the branch a hit takes behind its lights
NONE, MIRROR, ENTER, LEAVE, TIR = 0, 1, 2, 3, 4
# what happened anywhere in a ray's tree (bits of Shaded.events)
EV_SHADOW_NEAR, EV_SHADOW_BEYOND, EV_LIT_BACK, EV_LIT_FRONT, EV_ENTER, EV_LEAVE, EV_TIR, EV_DEPTH11, EV_MISS_DEEP, EV_GLOSSY_Z, EV_GLOSSY_XY = (
    1 << k for k in range(11))
EVENTS = ("shadow_near", "shadow_beyond", "lit_back", "lit_front", "enter", "leave", "tir", "depth11", "miss_deep", "glossy_z", "glossy_xy")
MAX_RECURSION_DEPTH = 10


class TooManyCasts(Exception):
    pass


class Shaded:
    """color: three mpf at the working precision. margin: the smallest of the tree. node, branch: of the depth-0 hit (-1, NONE on a miss). shadowed:
    bit l set when light l is shadowed at depth 0; shadowed_beyond: by occluders beyond the light only. path: every decision of the tree in order."""
    __slots__ = ("color", "margin", "node", "branch", "shadowed", "shadowed_beyond", "lit_front", "lit_back", "casts", "deepest", "depth11", "events", "path")

    def rgb(self):
        return [float(c) for c in self.color]


class _Tree:
    def __init__(self, draws, max_casts):
        self.draws, self.max_casts = draws, max_casts
        self.margin = math.inf
        self.casts = self.deepest = self.events = 0
        self.depth11 = False
        self.node, self.branch, self.shadowed, self.shadowed_beyond, self.lit_front, self.lit_back = -1, NONE, 0, 0, 0, 0
        self.path = []

    def note(self, m):
        if m != m:
            self.margin = 0.0
        elif m < self.margin:
            self.margin = m

    def cmp(self, a, b):
        self.note(_margin(a, b))

    def draw(self):
        return mpf(float(self.draws()))


def materials_of(scene):
    """The materials of the flattened nodes, breadth first (flat_scene.rs:22-38), as exact_ref.ExactScene numbers them."""
    out, queue = [], deque([scene.root])
    while queue:
        n = queue.popleft()
        if n.geometry is not None:
            out.append(n.geometry[1])
        queue.extend(n.children)
    return out


def _vec(v):
    return tuple(mpf(float(x)) for x in v)


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def _mulc(a, b):
    return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def _refracted_direction(st, ray_dir, normal, eta):
    """material.rs:27-48; None on total internal reflection."""
    eta_outside = mpf(1)
    ray_dot_norm = _dot(ray_dir, normal)
    under_sqrt = 1 - eta_outside * eta_outside * (1 - ray_dot_norm * ray_dot_norm) / (eta * eta)
    st.cmp(under_sqrt, mpf(0))
    if under_sqrt < 0:
        return None
    d1 = tuple(eta_outside * c / eta for c in _sub(ray_dir, _scale(normal, ray_dot_norm)))
    d2 = _scale(normal, mp.sqrt(under_sqrt))
    return _sub(d1, d2)


def _ray_color(ex, st, origin, direction, background, depth, mode, prec):
    """ray.rs:139-148."""
    st.casts += 1
    if st.casts > st.max_casts:
        raise TooManyCasts()
    h = ex.cast(origin, direction, mode=mode, prec=prec)
    st.note(h.margin)
    if not h:
        st.path.append(-1)
        if depth >= 1:
            st.events |= EV_MISS_DEEP
        return background
    st.path.append(h.node)
    return _hit_color(ex, st, h, direction, background, depth, mode, prec)


def _hit_color(ex, st, h, ray_dir, background, depth, mode, prec):
    """material.rs:91-320 without textures and normal maps."""
    if depth > MAX_RECURSION_DEPTH:
        st.depth11 = True
        st.events |= EV_DEPTH11
        return background
    st.deepest = max(st.deepest, depth)
    sh = ex.shading()
    m = sh["materials"][h.node]
    view = (-ray_dir[0], -ray_dir[1], -ray_dir[2])
    normal = h.normal   # normal.normalized(): cast() normalised it at this precision, and never turns it towards the viewer
    hit_point = h.point
    if any(c != c for c in normal):
        st.margin = 0.0
        return background
    if depth == 0:
        st.node = h.node
    diffuse_color = m["diffuse"]
    color = _mulc(sh["ambient"], diffuse_color)
    for li, light in enumerate(sh["lights"]):
        if light["point"]:
            light_pos = light["position"]
        else:   # light.rs:62-70, 88-90
            a_coord = 2 * st.draw() - 1
            b_coord = 2 * st.draw() - 1
            light_pos = _add(light["position"], _add(_scale(light["a"], a_coord), _scale(light["b"], b_coord)))
        hit_to_light = _sub(light_pos, hit_point)
        light_dist = mp.sqrt(_dot(hit_to_light, hit_to_light))
        if light_dist == 0:
            st.margin = 0.0
            return background
        light_dir = tuple(c / light_dist for c in hit_to_light)
        c0, c1, c2 = light["falloff"]
        attenuation = c0 + c1 * light_dist + c2 * light_dist * light_dist   # light.rs:32
        st.casts += 1
        if st.casts > st.max_casts:
            raise TooManyCasts()
        shadow = ex.cast(hit_point, light_dir, mode=mode, prec=prec)   # material.rs:176: [EPSILON, INFINITY), whatever the light's distance
        st.note(shadow.margin)
        st.path.append(bool(shadow))
        if shadow:
            beyond = shadow.t >= light_dist   # the nearest occluder lies beyond the light, so all do
            st.events |= EV_SHADOW_BEYOND if beyond else EV_SHADOW_NEAR
            if depth == 0:
                st.shadowed |= 1 << li
                if beyond:
                    st.shadowed_beyond |= 1 << li
            continue
        n_dot_l = _dot(normal, light_dir)
        if n_dot_l != 0:
            st.events |= EV_LIT_FRONT if n_dot_l > 0 else EV_LIT_BACK
            if depth == 0:
                if n_dot_l > 0:
                    st.lit_front |= 1 << li
                else:
                    st.lit_back |= 1 << li
        normal_light = n_dot_l if n_dot_l > 0 else mpf(0)
        diffuse = _scale(_mulc(diffuse_color, light["color"]), normal_light)
        if any(v > mpf(EPS_F64) for v in m["specular"]):
            half = _add(view, light_dir)
            hl = mp.sqrt(_dot(half, half))
            if hl == 0:
                st.margin = 0.0
                return background
            half = tuple(c / hl for c in half)
            nh = _dot(normal, half)
            nh = nh if nh > 0 else mpf(0)
            normal_half_shiny = mp.power(nh, 4 * m["shininess"]) if nh > 0 else (mpf(1) if m["shininess"] == 0 else mpf(0))
            specular = _scale(_mulc(m["specular"], light["color"]), normal_half_shiny)
        else:
            specular = (mpf(0), mpf(0), mpf(0))
        color = _add(color, tuple(c / attenuation for c in _add(diffuse, specular)))

    branch = NONE
    if m["reflectivity"] > 0:
        ray_dot_normal = _dot(ray_dir, normal)
        reflect_dir = _sub(ray_dir, _scale(_scale(normal, mpf(2)), ray_dot_normal))
        if m["glossy"] > 0:
            eps = mpf(EPS_F64)
            st.cmp(abs(reflect_dir[0]), eps)
            z_aligned = abs(reflect_dir[0]) < eps
            if z_aligned:   # && evaluates its right side only then
                st.cmp(abs(reflect_dir[1]), eps)
                z_aligned = abs(reflect_dir[1]) < eps
            tenth = mpf(0.1)
            if z_aligned:
                st.events |= EV_GLOSSY_Z
                offset_vector = _add(reflect_dir, (mpf(0), tenth, mpf(0)))
            else:
                st.events |= EV_GLOSSY_XY
                offset_vector = _add(reflect_dir, (mpf(0), mpf(0), tenth))
            st.path.append(bool(z_aligned))
            u_basis = _cross(reflect_dir, offset_vector)
            v_basis = _cross(reflect_dir, u_basis)
            g = m["glossy"]
            u_coord = -g / 2 + st.draw() * g
            v_coord = -g / 2 + st.draw() * g
            reflect_dir = _add(reflect_dir, _add(_scale(u_basis, u_coord), _scale(v_basis, v_coord)))
        reflected_color = _ray_color(ex, st, hit_point, reflect_dir, background, depth + 1, mode, prec)
        if m["ior"] > 0:
            st.cmp(ray_dot_normal, mpf(0))
            refract_dir = cos_incident = None
            if ray_dot_normal < 0:   # entering
                branch = ENTER
                refract_dir = _refracted_direction(st, ray_dir, normal, m["ior"])
                if refract_dir is None:   # the expect() of material.rs:257-258 panics
                    st.margin = 0.0
                    return background
                cos_incident = -ray_dot_normal   # (-ray_dir).dot(normal)
            else:
                refract_dir = _refracted_direction(st, ray_dir, (-normal[0], -normal[1], -normal[2]), 1 / m["ior"])
                if refract_dir is not None:
                    branch = LEAVE
                    cos_incident = _dot(refract_dir, normal)
                else:
                    branch = TIR
                    color = _add(color, _scale(reflected_color, m["reflectivity"]))
            st.events |= {ENTER: EV_ENTER, LEAVE: EV_LEAVE, TIR: EV_TIR}[branch]
            st.path.append(branch)
            if depth == 0:
                st.branch = branch
            if refract_dir is not None:
                ior = m["ior"]
                r0 = (ior - 1) * (ior - 1)
                r0 = r0 / ((ior + 1) * (ior + 1))
                x = 1 - cos_incident
                x5 = x * x * x * x * x   # powi(5)
                reflectivity = r0 + (1 - r0) * x5
                transmittance = 1 - reflectivity
                refracted_color = _ray_color(ex, st, hit_point, refract_dir, background, depth + 1, mode, prec)
                total = _add(_scale(reflected_color, reflectivity), _scale(refracted_color, transmittance))
                color = _add(color, _scale(total, m["reflectivity"]))
        else:
            branch = MIRROR
            if depth == 0:
                st.branch = branch
            color = _add(color, _scale(reflected_color, m["reflectivity"]))
    return color


class ExactScene(exact_ref.ExactScene):
    """exact_ref.ExactScene with the scene's shading: color() is Ray::color at depth 0."""

    def shading(self):
        """The scene's materials, lights and ambient colour at the working precision (f64 inputs taken as exact)."""
        key = mp.prec
        cache = self.__dict__.setdefault("_shading", {})
        if key not in cache:
            mats = []
            for m in materials_of(self.scene):
                if m.texture is not None or m.normals is not None or tuple(map(float, m.uv_trans)) != (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0):
                    raise ValueError("textures, normal maps and uv_trans are out of scope")
                mats.append(dict(diffuse=_vec(m.diffuse), specular=_vec(m.specular), shininess=mpf(float(m.shininess)), reflectivity=mpf(float(m.reflectivity)),
                                 glossy=mpf(float(m.glossy_side_length)), ior=mpf(float(m.refraction_index))))
            lights = []
            for l in self.scene.lights:
                a, b = tuple(map(float, l.area_a)), tuple(map(float, l.area_b))
                lights.append(dict(position=_vec(l.position), color=_vec(l.color), falloff=_vec(l.falloff), a=_vec(a), b=_vec(b),
                                   point=a == (0.0, 0.0, 0.0) or b == (0.0, 0.0, 0.0)))   # light.rs:51-53
            cache[key] = dict(materials=mats, lights=lights, ambient=_vec(self.scene.ambient))
        return cache[key]

    def color(self, origin, direction, background, draws=None, mode="flat", prec=PREC, max_casts=1 << 30):
        """Ray::color at depth 0: a Shaded. `draws()` yields the ray's next random number (needed only where the scene draws)."""
        old = mp.prec
        mp.prec = prec
        try:
            def none():
                raise ValueError("this scene draws random numbers: pass draws")
            st = _Tree(draws or none, max_casts)
            as_mpf = lambda v: tuple(x if isinstance(x, mpf) else mpf(float(x)) for x in v)
            c = _ray_color(self, st, as_mpf(origin), as_mpf(direction), as_mpf(background), 0, mode, prec)
            if any(x != x for x in c):
                st.margin = 0.0
            out = Shaded()
            out.color = tuple(+x for x in c)
            for k in ("margin", "node", "branch", "shadowed", "shadowed_beyond", "lit_front", "lit_back", "casts", "deepest", "depth11", "events", "path"):
                setattr(out, k, getattr(st, k))
            return out
        finally:
            mp.prec = old
