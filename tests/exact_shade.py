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

Textures, normal maps and uv_trans are restated from material.rs:113-143, texture.rs:104-221 and the primitives' tex_coord / normal_map_transform
(sphere.rs:58-96, cube.rs:46-137, plane.rs:40-46, triangle.rs:82-138, mesh.rs:100-112), see _maps(). A texel lookup's two truncations are comparisons
like any other: each records |x - nearest integer| / max(1, |x|) of the untruncated product u * (w - 1), so a lookup within 2^-30 of a texel edge makes
the ray fragile. atan2 and acos are mpmath's. A basis that is not finite (the sphere's pole, a triangle whose `coeff` is 0) is margin 0.

Out of scope: KDMesh, FnTex, image decoding (a texture is its decoded bytes).
"""
from __future__ import annotations

import math
from collections import deque

from mpmath import mp, mpf

import exact_ref
from exact_ref import EPS_F64, FRAGILE, PREC, _cross, _dot, _lt, _margin  # noqa: F401
from scene_dsl import CONE, CUBE, CYLINDER, MESH, PLANE, SPHERE, TRIANGLE

# the branch a hit takes behind its lights
NONE, MIRROR, ENTER, LEAVE, TIR = 0, 1, 2, 3, 4
# what happened anywhere in a ray's tree (bits of Shaded.events)
EV_SHADOW_NEAR, EV_SHADOW_BEYOND, EV_LIT_BACK, EV_LIT_FRONT, EV_ENTER, EV_LEAVE, EV_TIR, EV_DEPTH11, EV_MISS_DEEP, EV_GLOSSY_Z, EV_GLOSSY_XY = (
    1 << k for k in range(11))
EVENTS = ("shadow_near", "shadow_beyond", "lit_back", "lit_front", "enter", "leave", "tir", "depth11", "miss_deep", "glossy_z", "glossy_xy")
MAX_RECURSION_DEPTH = 10
GAMMA = 2.2   # math.rs:20, the f64 nearest to 2.2
# what the maps did anywhere in a ray's tree (bits of Shaded.tex_events): a texel fetched / a normal map applied per primitive kind, the cube face a
# mapped hit lies on, the to-top branch a normal-mapped sphere or cube took, a coordinate in (-1, 0) (truncated to 0, not floored to -1), a coordinate
# that truncates to exactly w - 1 from u >= 1 (modulo w keeps it, modulo w - 1 would not), one that truncates to w or more, a mapped hit at depth >= 1,
# a shading normal from a normal map that faces away from the viewer
TEX_EVENTS = ("tex_sphere", "tex_cube", "tex_plane", "tex_triangle", "tex_mesh", "nmap_sphere", "nmap_cube", "nmap_plane", "nmap_triangle", "nmap_mesh",
              "face_right", "face_left", "face_top", "face_bottom", "face_near", "face_far", "to_top_special", "to_top_general",
              "trunc_negative", "last_texel_from_above", "wrap_above", "mapped_deep", "nmap_faces_away")
_KIND_SLOT = {SPHERE: 0, CUBE: 1, PLANE: 2, TRIANGLE: 3, MESH: 4}


class TooManyCasts(Exception):
    pass


class Shaded:
    """color: three mpf at the working precision. margin: the smallest of the tree. node, branch: of the depth-0 hit (-1, NONE on a miss). shadowed:
    bit l set when light l is shadowed at depth 0; shadowed_beyond: by occluders beyond the light only. path: every decision of the tree in order."""
    __slots__ = ("color", "margin", "node", "branch", "shadowed", "shadowed_beyond", "lit_front", "lit_back", "casts", "deepest", "depth11", "events", "path",
                 "tex_events", "tex0")

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
        self.tex_events = 0
        self.tex0 = None   # the depth-0 hit's lookups: see _maps()

    def tex(self, name):
        self.tex_events |= 1 << TEX_EVENTS.index(name)

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


def _normalized(v):
    """vek's normalized(): self / self.magnitude(); a zero vector gives 0 / 0."""
    s = _dot(v, v)
    if s == 0 or s != s:
        return (mp.nan, mp.nan, mp.nan)
    r = mp.sqrt(s)
    return (v[0] / r, v[1] / r, v[2] / r)


def _cols(c0, c1, c2, v):
    """Mat3::from_col_arrays([c0, c1, c2]) * v."""
    return tuple(c0[q] * v[0] + c1[q] * v[1] + c2[q] * v[2] for q in range(3))


# cube.rs:46-65: (uv axis direction, uv offset) of right, left, top, bottom, near, far, in the order of exact_ref._CUBE_FACES
def _cube_faces():
    third, f = mpf(1) / 3, mpf
    return (((f(-1), f(1)), (f(1) / 2, third)), ((f(1), f(1)), (f(0), third)), ((f(1), f(-1)), (f(1) / 4, f(0))),
            ((f(1), f(1)), (f(1) / 4, f(2) / 3)), ((f(1), f(1)), (f(1) / 4, third)), ((f(-1), f(1)), (f(3) / 4, third)))


def _to_top_basis(st, p, normal, top):
    """sphere.rs:79-96 / cube.rs:119-135: the basis from `to_top`, top = RADIUS or L (both 1)."""
    to_top = _normalized((-p[0], mpf(top) - p[1], -p[2]))
    if to_top[0] != to_top[0]:
        st.margin = 0.0
        return None, to_top
    eps = mpf(EPS_F64)
    special = _lt(st, abs(to_top[0]), eps)
    if special:   # && evaluates its right side only then
        special = _lt(st, abs(to_top[2]), eps)
    if special:
        st.tex("to_top_special")
        third = (mpf(0), mpf(0), mpf(1)) if normal[1] > 0 else (mpf(0), mpf(0), mpf(-1))   # back_rh, forward_rh
        st.cmp(normal[1], mpf(0))
        return ((mpf(1), mpf(0), mpf(0)), normal, third), to_top
    st.tex("to_top_general")
    horizontal_tangent = _cross(to_top, normal)
    vertical_tangent = _cross(normal, horizontal_tangent)
    return (horizontal_tangent, normal, vertical_tangent), to_top


def _surface_maps(ex, st, h, want_basis):
    """The hit's tex_coord and, if wanted, its normal_map_transform (three columns, or None when it is not finite), in the primitive's model space.
    Returns (u, v), basis, to_top."""
    p = h.model_point
    geo = ex.flat[h.node].geometry
    basis = to_top = None
    if h.kind == SPHERE:   # sphere.rs:58-96
        if p[2] == 0 and p[0] <= 0 or abs(p[1]) > 1:   # atan2's cut (the sign of an IEEE zero is not represented here); acos outside [-1, 1] is NaN
            st.margin = 0.0
            return None, None, None
        u = (mp.pi + mp.atan2(-p[2], p[0])) / (2 * mp.pi)
        v = mp.acos(p[1]) / mp.pi
        if want_basis:
            basis, to_top = _to_top_basis(st, p, p, 1)
    elif h.kind == CUBE:   # cube.rs:84-137: the face the fold kept is h.part
        axis, _sign = exact_ref._CUBE_FACES[h.part]
        uv_axis, uv_offset = _cube_faces()[h.part]
        face_u, face_v = ((p[2], p[1]), (p[0], p[2]), (p[0], p[1]))[axis]
        half = mpf(0.5)
        norm_u, norm_v = face_u * uv_axis[0] + half, half - face_v * uv_axis[1]
        u, v = norm_u / 4 + uv_offset[0], norm_v / 3 + uv_offset[1]
        st.tex(TEX_EVENTS[10 + h.part])
        if want_basis:
            n = [mpf(0), mpf(0), mpf(0)]
            n[axis] = mpf(_sign)
            basis, to_top = _to_top_basis(st, p, tuple(n), 1)
    elif h.kind == PLANE:   # plane.rs:40-46
        u, v = p[0] + mpf(0.5), p[2] + mpf(0.5)
        basis = ((mpf(1), mpf(0), mpf(0)), (mpf(0), mpf(1), mpf(0)), (mpf(0), mpf(0), mpf(1)))
    elif h.kind in (TRIANGLE, MESH):   # triangle.rs:82-138 (mesh.rs:100-112 hands the mesh's arrays over per triangle)
        prim = geo.prim
        if h.kind == TRIANGLE:
            va, vb, vc, normals = geo.data()
            tc = prim.tri_tex_coords
        else:
            pos, nrm, tris, _, _ = geo.data()
            ia, ib, ic = tris[h.sub]
            va, vb, vc = pos[ia], pos[ib], pos[ic]
            normals = None if nrm is None else (nrm[ia], nrm[ib], nrm[ic])
            tc = None if prim.mesh.tex_coords is None else [prim.mesh.tex_coords[q] for q in (ia, ib, ic)]
        if tc is None:
            raise ValueError("a triangle without texture coordinates under a mapped material: the reference panics (material.rs:134, 142)")
        uv_a, uv_b, uv_c = ((mpf(float(t[0])), mpf(float(t[1]))) for t in tc)
        beta, gamma = h.bary
        alpha = 1 - beta - gamma
        uv = tuple(uv_a[q] * alpha + uv_b[q] * beta + uv_c[q] * gamma for q in range(2))
        u, v = uv[0], 1 - uv[1]   # triangle.rs:99: v is reversed here, and only here
        if want_basis:
            if normals is not None:
                normal = tuple(normals[0][q] * alpha + normals[1][q] * beta + normals[2][q] * gamma for q in range(3))
            else:
                normal = _cross(exact_ref._sub(vb, va), exact_ref._sub(vc, va))
            edge1, edge2 = exact_ref._sub(vb, va), exact_ref._sub(vc, va)
            d1 = (uv_b[0] - uv_a[0], uv_b[1] - uv_a[1])
            d2 = (uv_c[0] - uv_a[0], uv_c[1] - uv_a[1])
            tangent = tuple(d2[1] * edge1[q] - d1[1] * edge2[q] for q in range(3))
            bitangent = tuple(-d2[0] * edge1[q] + d1[0] * edge2[q] for q in range(3))
            coeff = d1[0] * d2[1] - d2[0] * d1[1]
            if coeff == 0:
                basis = None
                st.margin = 0.0
            else:
                basis = (_normalized(tuple(c / coeff for c in tangent)), _normalized(normal), _normalized(tuple(c / coeff for c in bitangent)))   # the MODEL-space normal
    else:
        raise ValueError("primitive kind %d has no texture coordinates: the reference panics (material.rs:134, 142)" % h.kind)
    if basis is not None and any(c != c for col in basis for c in col):
        basis = None
        st.margin = 0.0
    return (u, v), basis, to_top


def _texel(st, image, u, v):
    """RgbImageBuffer::at (texture.rs:104-141): the texel's bytes, its indices and the smaller of the two truncations' margins."""
    height, width = image.shape[0], image.shape[1]
    idx, raw, margin = [], [], math.inf
    for coord, size in ((u, width), (v, height)):
        x = coord * mpf(size - 1)
        if x != x:
            st.margin = 0.0
            return None
        nearest = mp.nint(x)
        m = float(abs(x - nearest)) / max(1.0, abs(float(x)))   # `as i64` decides by which side of an integer the product lies
        st.note(m)
        margin = min(margin, m)
        _lt(st, x, mpf(0))                                           # rem_euclid's sign test, on the product it truncates
        t = int(mp.floor(x)) if x >= 0 else -int(mp.floor(-x))      # `as i64` truncates toward zero
        if -1 < x < 0:
            st.tex("trunc_negative")
        if coord >= 1 and t == size - 1:
            st.tex("last_texel_from_above")
        if t >= size:
            st.tex("wrap_above")
        r = abs(t) % size   # value % rhs keeps the sign of value
        r = -r if t < 0 else r
        if r < 0:
            r += size
        idx.append(r)
        raw.append(x)
    px = image[idx[1], idx[0]]
    return (int(px[0]), int(px[1]), int(px[2])), idx, margin


def _maps(ex, st, h, m, view, depth):
    """material.rs:113-143: (shading normal or None, diffuse colour). The shading normal from a normal map is norm_trans * tex_norm.normalized() with
    nothing after it (:133): not normalised, and the hit's world-space normal, the only thing the nodes' normal_trans touched, is not used at all."""
    texture, normals = m["texture"], m["normals"]
    slot = _KIND_SLOT.get(h.kind)
    uv, basis, to_top = _surface_maps(ex, st, h, normals is not None)
    if uv is None:
        return None, None
    t = m["uv_trans"]   # :113-117: uv_trans * (u, v, 1); Vec2::from drops the third component
    tu = t[0] * uv[0] + t[1] * uv[1] + t[2]
    tv = t[3] * uv[0] + t[4] * uv[1] + t[5]
    if depth >= 1:
        st.tex("mapped_deep")
    rec = dict(kind=h.kind, face=h.part if h.kind == CUBE else -1, uv=uv, tuv=(tu, tv), to_top=to_top, texel=None, nmap_texel=None, bary=h.bary, margin=math.inf)
    normal = None
    if normals is not None:   # :126-136
        if basis is None:
            return None, None
        got = _texel(st, normals, tu, tv)
        if got is None:
            return None, None
        (r, g, b), idx, rec["margin"] = got
        rec["nmap_texel"] = (idx[0], idx[1], r, g, b)
        st.path.append(("normal texel", idx[0], idx[1]))
        c = [mpf(x) / 255 for x in (r, g, b)]
        norm = (2 * c[0] - 1, 2 * c[1] - 1, -(2 * c[2] - 1))   # texture.rs:204-208
        tex_norm = (norm[0], -norm[2], -norm[1])                # normal_to_rh (:217-221)
        normal = _cols(basis[0], basis[1], basis[2], _normalized(tex_norm))
        st.tex(TEX_EVENTS[5 + slot])
        if _dot(normal, view) < 0:
            st.tex("nmap_faces_away")
    diffuse = m["diffuse"]
    if texture is not None:   # :138-144, texture.rs:162-168
        got = _texel(st, texture, tu, tv)
        if got is None:
            return None, None
        (r, g, b), idx, margin = got
        rec["margin"] = min(rec["margin"], margin)
        rec["texel"] = (idx[0], idx[1], r, g, b)
        st.path.append(("texel", idx[0], idx[1]))
        diffuse = tuple(mp.power(mpf(x) / 255, mpf(GAMMA)) for x in (r, g, b))
        st.tex(TEX_EVENTS[slot])
    if depth == 0:
        st.tex0 = rec
    return normal, diffuse


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
    """material.rs:91-320."""
    if depth > MAX_RECURSION_DEPTH:
        st.depth11 = True
        st.events |= EV_DEPTH11
        return background
    st.deepest = max(st.deepest, depth)
    sh = ex.shading()
    m = sh["materials"][h.node]
    view = (-ray_dir[0], -ray_dir[1], -ray_dir[2])
    normal = h.normal   # material.rs:124, normal.normalized(): cast() normalised it at this precision, and never turns it towards the viewer
    hit_point = h.point
    diffuse_color = m["diffuse"]
    if m["texture"] is not None or m["normals"] is not None:
        mapped_normal, diffuse_color = _maps(ex, st, h, m, view, depth)
        if diffuse_color is None:   # a lookup that cannot be decided
            st.margin = 0.0
            return background
        if mapped_normal is not None:   # material.rs:126-136: replaces the world-space normal, which went through normal_trans, altogether
            normal = mapped_normal
    if any(c != c for c in normal):
        st.margin = 0.0
        return background
    if depth == 0:
        st.node = h.node
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
            for node, m in zip(self.flat, materials_of(self.scene)):
                mapped = m.texture is not None or m.normals is not None
                if mapped and node.geometry.kind in (CONE, CYLINDER):
                    raise ValueError("a cone or cylinder under a mapped material: the reference panics (material.rs:134, 142)")
                mats.append(dict(diffuse=_vec(m.diffuse), specular=_vec(m.specular), shininess=mpf(float(m.shininess)), reflectivity=mpf(float(m.reflectivity)),
                                 glossy=mpf(float(m.glossy_side_length)), ior=mpf(float(m.refraction_index)),
                                 texture=None if m.texture is None else m.texture.pixels, normals=None if m.normals is None else m.normals.pixels,
                                 uv_trans=tuple(mpf(float(x)) for x in m.uv_trans)))   # without a map the coordinate is transformed and never read
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
            for k in ("margin", "node", "branch", "shadowed", "shadowed_beyond", "lit_front", "lit_back", "casts", "deepest", "depth11", "events", "path",
                      "tex_events", "tex0"):
                setattr(out, k, getattr(st, k))
            return out
        finally:
            mp.prec = old
