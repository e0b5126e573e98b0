"""PBRT-v4's disk and cylinder (ShmSphere.quadric; shimmer_amd/csrc/shm/shapes.h, quadric_*) restated in float64 NumPy, and the records and rays the CPU tests
(tests/test_quadrics.py, against the oracle) and the GPU tests (tests/test_gpu_quadrics.py, the leaf probes against the oracle) share. Written from the definitions —
PBRT-v4 shapes.h / shapes.cpp, with the one stated deviation: an area sample is drawn from the annulus sector the disk is, not from the whole disk — and not from the
C++: plain real arithmetic, no intervals, no refinement of a hit point (which moves it by rounding errors only)."""
import numpy as np

from shimmer_amd import abi

TWO_PI = 2.0 * np.pi


def record(kind, radius=1.0, z_min=0.0, z_max=0.0, inner=0.0, phi_max_deg=360.0, m=None, reverse=False):
    """A ShmSphere of the kind as the builders write it; m: render_from_object (4 x 4), default the identity."""
    s = abi.ShmSphere()
    s.quadric = {"disk": abi.SHM_QUADRIC_DISK, "cylinder": abi.SHM_QUADRIC_CYLINDER}[kind]
    s.radius, s.z_min, s.z_max = radius, z_min, z_max if kind == "cylinder" else z_min
    s.theta_z_min, s.theta_z_max = inner, 0.0
    s.phi_max = float(np.float32(np.pi / 180.0) * np.float32(phi_max_deg))
    m = np.eye(4) if m is None else np.asarray(m, np.float64)
    s.render_from_object[:] = [float(x) for x in m.astype(np.float32).ravel()]
    s.object_from_render[:] = [float(x) for x in np.linalg.inv(m).astype(np.float32).ravel()]
    s.reverse_orientation = int(reverse)
    s.transform_swaps_handedness = int(np.linalg.det(m[:3, :3]) < 0)
    return s


def _mats(s):
    return (np.array(list(s.render_from_object), np.float64).reshape(4, 4), np.array(list(s.object_from_render), np.float64).reshape(4, 4))


def area(s):
    if s.quadric == abi.SHM_QUADRIC_DISK:
        return s.phi_max * (s.radius ** 2 - s.theta_z_min ** 2) / 2.0
    return (s.z_max - s.z_min) * s.radius * s.phi_max


def _phi(x, y):
    phi = np.arctan2(y, x)
    return phi + TWO_PI if phi < 0 else phi


def intersect(s, ro, rd, t_max=np.inf):
    """-> None or (t, p_obj, phi): the first root that survives the clipping, the second one if the first is clipped."""
    rfo, ofr = _mats(s)
    o = ofr[:3, :3] @ np.asarray(ro, np.float64) + ofr[:3, 3]
    d = ofr[:3, :3] @ np.asarray(rd, np.float64)
    if s.quadric == abi.SHM_QUADRIC_DISK:
        if d[2] == 0.0:
            return None
        t = (s.z_min - o[2]) / d[2]
        if not (0.0 < t < t_max):
            return None
        p = o + t * d
        d2 = p[0] ** 2 + p[1] ** 2
        if d2 > s.radius ** 2 or d2 < s.theta_z_min ** 2:
            return None
        phi = _phi(p[0], p[1])
        return None if phi > s.phi_max else (t, p, phi)
    a = d[0] ** 2 + d[1] ** 2
    if a == 0.0:
        return None
    b = 2.0 * (d[0] * o[0] + d[1] * o[1])
    c = o[0] ** 2 + o[1] ** 2 - s.radius ** 2
    disc = b * b - 4.0 * a * c
    if disc < 0.0:
        return None
    roots = sorted(((-b - np.sqrt(disc)) / (2 * a), (-b + np.sqrt(disc)) / (2 * a)))
    if roots[0] > t_max or roots[1] <= 0.0:
        return None
    for t in roots:
        if t <= 0.0:
            continue
        if t > t_max:
            return None
        p = o + t * d
        phi = _phi(p[0], p[1])
        if not (p[2] < s.z_min or p[2] > s.z_max or phi > s.phi_max):
            return (t, p, phi)
    return None


def interaction(s, p, phi):
    """-> dict(p, n, uv, dpdu, dpdv) in render space: the point, the geometric normal (flipped by reverse_orientation ^ transform_swaps_handedness), (u, v) and the
    two derivatives, as PBRT-v4's Transform::operator()(SurfaceInteraction) takes them there."""
    rfo, ofr = _mats(s)
    p = np.array(p, np.float64)
    u = phi / s.phi_max
    dpdu = np.array([-s.phi_max * p[1], s.phi_max * p[0], 0.0])
    if s.quadric == abi.SHM_QUADRIC_DISK:
        r_hit = np.hypot(p[0], p[1])
        v = (s.radius - r_hit) / (s.radius - s.theta_z_min)
        dpdv = np.array([p[0], p[1], 0.0]) * (s.theta_z_min - s.radius) / r_hit
        p[2] = s.z_min
    else:
        v = (p[2] - s.z_min) / (s.z_max - s.z_min)
        dpdv = np.array([0.0, 0.0, s.z_max - s.z_min])
    n = np.cross(dpdu, dpdv)
    n /= np.linalg.norm(n)
    if bool(s.reverse_orientation) ^ bool(s.transform_swaps_handedness):
        n = -n
    n_r = ofr[:3, :3].T @ n
    return dict(p=rfo[:3, :3] @ p + rfo[:3, 3], n=n_r / np.linalg.norm(n_r), uv=(u, v), dpdu=rfo[:3, :3] @ dpdu, dpdv=rfo[:3, :3] @ dpdv)


def sample(s, u):
    """The area sample -> (p, n) in render space; its density is 1 / area(s)."""
    rfo, ofr = _mats(s)
    phi = u[1] * s.phi_max
    if s.quadric == abi.SHM_QUADRIC_DISK:
        rho = np.sqrt((1.0 - u[0]) * s.theta_z_min ** 2 + u[0] * s.radius ** 2)
        p, n = np.array([rho * np.cos(phi), rho * np.sin(phi), s.z_min]), np.array([0.0, 0.0, 1.0])
    else:
        p = np.array([s.radius * np.cos(phi), s.radius * np.sin(phi), (1.0 - u[0]) * s.z_min + u[0] * s.z_max])
        n = np.array([p[0], p[1], 0.0])
    n = ofr[:3, :3].T @ n
    n /= np.linalg.norm(n)
    return rfo[:3, :3] @ p + rfo[:3, 3], (-n if s.reverse_orientation else n)


def sample_with_context(s, ctx_p, u):
    """-> None or (p, n, pdf with respect to solid angle at ctx_p)"""
    p, n = sample(s, u)
    wi = p - np.asarray(ctx_p, np.float64)
    d2 = float(wi @ wi)
    if d2 == 0.0:
        return None
    wi /= np.sqrt(d2)
    cos = abs(float(n @ -wi))
    if cos == 0.0:
        return None
    return p, n, (1.0 / area(s)) / (cos / d2)


def pdf_with_context(s, ctx_p, wi):
    hit = intersect(s, ctx_p, wi)
    if hit is None:
        return 0.0
    it = interaction(s, hit[1], hit[2])
    d2 = float(np.sum((it["p"] - np.asarray(ctx_p, np.float64)) ** 2))
    cos = abs(float(it["n"] @ -np.asarray(wi, np.float64)))
    return 0.0 if cos == 0.0 else (1.0 / area(s)) / (cos / d2)


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], np.float64)


def _at(m, t):
    m = np.array(m, np.float64)
    m[:3, 3] = t
    return m


# ---- the leaf cases: name -> (record, ray origin, ray direction, t_max, hit expected) ----
_NONUNIFORM = _at(_rot_x(0.4) @ np.diag([1.5, 0.6, 1.2, 1.0]), (0.2, -0.1, 0.3))
_MIRROR = _at(np.diag([1.0, 1.0, -1.0, 1.0]), (0.0, 0.0, 0.5))
INF = float("inf")
HIT_CASES = {
    "full disk": (record("disk", 1.0, 0.5), (0.3, 0.2, 3.0), (0.05, -0.1, -1.0), INF, True),
    "annulus, through the ring": (record("disk", 1.0, 0.0, inner=0.4), (0.7, 0.1, 2.0), (0.0, 0.0, -1.0), INF, True),
    "annulus, through the hole": (record("disk", 1.0, 0.0, inner=0.4), (0.1, 0.1, 2.0), (0.0, 0.0, -1.0), INF, False),
    "sector, inside phimax": (record("disk", 1.0, 0.0, phi_max_deg=200.0), (-0.5, 0.3, 1.0), (0.0, 0.0, -1.0), INF, True),
    "sector, beyond phimax": (record("disk", 1.0, 0.0, phi_max_deg=200.0), (0.5, -0.3, 1.0), (0.0, 0.0, -1.0), INF, False),
    "disk beyond the radius": (record("disk", 1.0, 0.0), (1.2, 0.0, 1.0), (0.0, 0.0, -1.0), INF, False),
    "disk from below": (record("disk", 1.0, 0.25), (0.2, -0.3, -2.0), (0.1, 0.05, 1.0), INF, True),
    "disk under a non-uniform scale": (record("disk", 0.8, 0.1, inner=0.1, m=_NONUNIFORM), (0.4, 0.3, 3.0), (-0.05, -0.1, -1.0), INF, True),
    "disk under a mirroring matrix": (record("disk", 0.9, 0.2, m=_MIRROR), (0.3, -0.4, 4.0), (0.02, 0.03, -1.0), INF, True),
    "disk with reverse_orientation": (record("disk", 0.9, 0.0, reverse=True), (0.3, -0.4, 4.0), (0.02, 0.03, -1.0), INF, True),
    "ray in the disk's plane": (record("disk", 1.0, 0.0), (-3.0, 0.1, 0.0), (1.0, 0.0, 0.0), INF, False),
    "disk behind t_max": (record("disk", 1.0, 0.0), (0.1, 0.1, 2.0), (0.0, 0.0, -1.0), 1.5, False),
    "cylinder from outside": (record("cylinder", 0.5, -1.0, 1.0), (3.0, 0.2, 0.3), (-1.0, 0.0, -0.1), INF, True),
    "cylinder from inside": (record("cylinder", 0.5, -1.0, 1.0), (0.1, 0.1, 0.0), (0.6, 0.7, 0.2), INF, True),
    "cylinder, first root clipped by z": (record("cylinder", 0.5, -1.0, 1.0), (2.0, 0.0, 2.6), (-1.0, 0.05, -1.0), INF, True),
    "cylinder, first root clipped by phi": (record("cylinder", 0.5, -1.0, 1.0, phi_max_deg=180.0), (0.1, -3.0, 0.2), (0.0, 1.0, 0.0), INF, True),
    "cylinder, both roots clipped": (record("cylinder", 0.5, -1.0, 1.0), (2.0, 0.0, 3.8), (-1.0, 0.0, -1.0), INF, False),
    "cylinder, ray parallel to the axis": (record("cylinder", 0.5, -1.0, 1.0), (0.5, 0.0, -3.0), (0.0, 0.0, 1.0), INF, False),
    "cylinder, t_max between the roots": (record("cylinder", 0.5, -1.0, 1.0), (3.0, 0.0, 0.0), (-1.0, 0.0, 0.0), 3.0, True),
    "cylinder, t_max between the roots, first clipped": (record("cylinder", 0.5, -1.0, 1.0, phi_max_deg=90.0), (0.2, -3.0, 0.0), (0.0, 1.0, 0.0), 3.0, False),
    "cylinder, t_max before the first root": (record("cylinder", 0.5, -1.0, 1.0), (3.0, 0.0, 0.0), (-1.0, 0.0, 0.0), 2.0, False),
    "cylinder missed": (record("cylinder", 0.5, -1.0, 1.0), (3.0, 2.0, 0.0), (-1.0, 0.0, 0.0), INF, False),
    "cylinder under a rotation and a scale": (record("cylinder", 0.4, 0.0, 1.5, phi_max_deg=300.0, m=_NONUNIFORM), (3.0, 0.5, 0.4), (-2.8, -0.95, 0.73), INF, True),
}
# ---- emitters seen from a reference point: name -> (record, ctx_p) ----
SAMPLE_CASES = {
    "disk on its axis": (record("disk", 0.6, 0.0), (0.0, 0.0, 1.2)),
    "annulus on its axis": (record("disk", 0.6, 0.0, inner=0.25), (0.0, 0.0, 0.9)),
    "sector on its axis": (record("disk", 0.6, 0.0, phi_max_deg=135.0), (0.0, 0.0, 0.7)),
    "disk off its axis, scaled": (record("disk", 0.8, 0.1, inner=0.1, m=_NONUNIFORM), (0.9, 0.6, 1.7)),
    "disk, mirrored": (record("disk", 0.9, 0.2, m=_MIRROR), (0.4, 0.2, 2.0)),
    "disk, reversed": (record("disk", 0.9, 0.0, reverse=True), (0.4, 0.2, 2.0)),
    "cylinder from outside": (record("cylinder", 0.5, -0.6, 0.8), (2.0, 0.3, 0.2)),
    "cylinder sector from inside": (record("cylinder", 0.5, -0.6, 0.8, phi_max_deg=240.0), (0.1, -0.05, 0.1)),
}
