"""Ray queries for the caller's rays (include/vkr_ray_queries.h): the record layouts, the numpy restatement of the rules
in the header's comment, the rays of the tests and the smallest end-to-end use,

    python -m vulkan_renderer_amd.ray_queries SCENE.vks --depth OUT.npy [--width W --height H]

which writes t of the camera's pixel-centre rays as a float32 array (infinity where nothing is hit).

The restatement is float32 throughout, one rounding per operation like the kernels (csrc/ray_queries.hip), vectorised
over triangles and chunked over rays: it is what the kernels' answers are compared with bit for bit, and it is itself
pinned against the oracle's closest front hit and any hit (tests/test_ray_queries.py)."""
import numpy as np

# ray_t, ray_hit_t
RAY = np.dtype([("origin", np.float32, 3), ("t_min", np.float32), ("direction", np.float32, 3), ("t_max", np.float32)])
HIT = np.dtype([("primitive", np.uint32), ("t", np.float32), ("u", np.float32), ("v", np.float32)])
# ray_walk_t
WALK = {"auto": 0, "binary": 1, "wide": 2}
NO_PRIMITIVE = 0xFFFFFFFF
# kWideStackLds, kWideStackMax of csrc/lbvh.h
WIDE_STACK_LDS, WIDE_STACK_MAX = 16, 128

_ONE, _MINUS_ONE, _ZERO = np.float32(1), np.float32(-1), np.float32(0)


def make_rays(origins, directions, t_min=1.0e-3, t_max=np.inf):
    """-> RAY records; origins and directions (n, 3), t_min and t_max scalars or (n,)"""
    origins = np.asarray(origins, np.float32).reshape(-1, 3)
    rays = np.zeros(len(origins), RAY)
    rays["origin"], rays["direction"] = origins, np.asarray(directions, np.float32).reshape(-1, 3)
    rays["t_min"], rays["t_max"] = t_min, t_max
    return rays


def misses():
    """-> one ray_hit_t of a miss"""
    out = np.zeros(1, HIT)
    out["primitive"], out["t"] = NO_PRIMITIVE, np.inf
    return out


def dequantize(quantized_positions, factor, summand):
    """The vertices of a scene file, (T, 3, 3) float32: 21 bits per coordinate in two words per vertex, then
    (float) q * factor + summand (oracle_bvh.c:84-92, reference scene.c:176-187)"""
    q = np.ascontiguousarray(quantized_positions, np.uint32).reshape(-1, 2)
    q0, q1 = q[:, 0], q[:, 1]
    p = np.stack([q0 & 0x1FFFFF, ((q0 & 0xFFE00000) >> 21) | ((q1 & 0x3FF) << 11), (q1 & 0x7FFFFC00) >> 10], -1).astype(np.float32)
    w = p * np.asarray(factor, np.float32) + np.asarray(summand, np.float32)
    return w.reshape(-1, 3, 3)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def degenerate(rays):
    """Rule 6: rays that miss whatever the triangles are"""
    floats = np.ascontiguousarray(rays).view(np.float32).reshape(-1, 8)
    return np.isnan(floats).any(axis=1) | ~(rays["t_max"] >= rays["t_min"]) | (rays["direction"] == 0).all(axis=1)


def passing_triangles(vertices, rays, cull_back_faces, chunk=128):
    """Rules 1 and 2 for every pair: yields (ray indices, triangle indices, t, u, v) of the triangles that pass, ray
    chunk by ray chunk"""
    vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3, 3)
    p0 = vertices[:, 0]
    e1, e2 = vertices[:, 1] - p0, vertices[:, 2] - p0
    walked = np.nonzero(~degenerate(rays))[0]
    with np.errstate(all="ignore"):
        for start in range(0, len(walked), chunk):
            index = walked[start:start + chunk]
            o, d = rays["origin"][index][:, None, :], rays["direction"][index][:, None, :]
            p = _cross(d, e2[None])
            det = _dot(e1[None], p)
            ok = (det > 0) if cull_back_faces else (det != 0)
            sign = np.where(det < 0, _MINUS_ONE, _ONE)
            adet = det * sign
            s = o - p0[None]
            U = _dot(s, p) * sign
            ok &= (U >= 0) & (U <= adet)
            # (the rest on the pairs that are left)
            r, k = np.nonzero(ok)
            sign, adet, U, s, d = sign[r, k], adet[r, k], U[r, k], s[r, k], d[r, 0]
            q = _cross(s, e1[k])
            V = _dot(d, q) * sign
            T = _dot(e2[k], q) * sign
            t_min, t_max = rays["t_min"][index][r], rays["t_max"][index][r]
            ok = (V >= 0) & (U + V <= adet) & (T >= t_min * adet) & (T <= t_max * adet)
            r, k, adet, U, V, T = r[ok], k[ok], adet[ok], U[ok], V[ok], T[ok]
            yield index[r], k, T / adet, U / adet, V / adet


def closest_hits_brute_force(vertices, rays, cull_back_faces):
    """Rules 3 and 4: HIT records, the passing triangle with the smallest (t, primitive) of every ray"""
    out = np.repeat(misses(), len(rays))
    for ray, primitive, t, u, v in passing_triangles(vertices, rays, cull_back_faces):
        # (NaNs sort behind every number)
        order = np.lexsort((primitive, t, ray))
        ray, first = np.unique(ray[order], return_index=True)
        winner = order[first]
        out["primitive"][ray], out["t"][ray], out["u"][ray], out["v"][ray] = primitive[winner], t[winner], u[winner], v[winner]
    return out


def closest_and_runner_up(vertices, rays, cull_back_faces):
    """-> (HIT records, t of the second smallest (t, primitive) of every ray, infinity if there is none): for tests that
    want to know how close a decision was"""
    out, second = np.repeat(misses(), len(rays)), np.full(len(rays), np.inf, np.float32)
    for ray, primitive, t, u, v in passing_triangles(vertices, rays, cull_back_faces):
        order = np.lexsort((primitive, t, ray))
        sorted_ray = ray[order]
        ray, first, count = np.unique(sorted_ray, return_index=True, return_counts=True)
        winner = order[first]
        out["primitive"][ray], out["t"][ray], out["u"][ray], out["v"][ray] = primitive[winner], t[winner], u[winner], v[winner]
        several = count > 1
        second[ray[several]] = t[order[first[several] + 1]]
    return out, second


def any_hits_brute_force(vertices, rays):
    """Rule 5: bool per ray"""
    out = np.zeros(len(rays), bool)
    for ray, _, _, _, _ in passing_triangles(vertices, rays, False):
        out[ray] = True
    return out


def test_rays(vertices, n, seed):
    """The rays of the tests: origins uniform in [-8, 8]^2 x [0.001, 2]; ray i has a normal-distributed direction
    (i mod 3 = 0), aims at a random vertex (1) or at the float32 midpoint of a random edge (2), the aimed directions
    un-normalised (t = 1 at the target: ties and edge-on cases by construction); t in [1e-3, 1e3]"""
    vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    origins = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(0.001, 2, n)], -1).astype(np.float32)
    directions = rng.standard_normal((n, 3)).astype(np.float32)
    triangle, corner = rng.integers(0, len(vertices), n), rng.integers(0, 3, n)
    vertex = vertices[triangle, corner]
    midpoint = (vertex + vertices[triangle, (corner + 1) % 3]) * np.float32(0.5)
    kind = np.arange(n) % 3
    directions[kind == 1] = (vertex - origins)[kind == 1]
    directions[kind == 2] = (midpoint - origins)[kind == 2]
    return make_rays(origins, directions, 1.0e-3, 1.0e3)


test_rays.__test__ = False  # (not a test, whatever collects this module)


def pixel_rays(constants, width, height, near, far):
    """The pixel-centre rays of k_primary_visibility (csrc/render_targets.hip), raster order, from the bytes of the
    constant buffer: pixel_to_ray_direction_world_space at 96 ... 140, the camera position at 144 ... 152; float32 in
    the same operation order.  The direction has view-space depth 1, so [near, far] is the parameter range."""
    c = np.ascontiguousarray(constants, np.uint8)
    m = c[96:144].view(np.float32).reshape(3, 4)
    origin = c[144:156].view(np.float32)
    fy, fx = np.meshgrid(np.arange(height, dtype=np.float32), np.arange(width, dtype=np.float32), indexing="ij")
    direction = np.stack([(m[j, 0] * fx + m[j, 1] * fy) + m[j, 2] for j in range(3)], -1).reshape(-1, 3)
    return make_rays(np.broadcast_to(origin, direction.shape), direction, near, far)


def main(argv=None):
    import argparse

    from . import renderer, synthetic
    parser = argparse.ArgumentParser(description="Depth of the camera rays of a scene, traced on the device")
    parser.add_argument("scene", help="a *.vks scene")
    parser.add_argument("--depth", required=True, help="the float32 array (height, width) to write, *.npy")
    parser.add_argument("--width", type=int, default=640)
    parser.add_argument("--height", type=int, default=360)
    args = parser.parse_args(argv)
    r = renderer.Renderer()
    try:
        r.load_scene(args.scene, acceleration_structure=True)
        camera = synthetic.DEFAULT_CAMERA
        r.set_camera(camera["position"], camera["rotation_x"], camera["rotation_z"], camera["vertical_fov"])
        r.app.swapchain.extent.width, r.app.swapchain.extent.height = args.width, args.height
        rays = r.pixel_rays()
        hits = r.trace_closest_hits(rays["origin"], rays["direction"], rays["t_min"], rays["t_max"], cull_back_faces=True)
    finally:
        r.close()
    depth = hits["t"].reshape(args.height, args.width)
    np.save(args.depth, depth)
    print("%s: %d x %d, %.1f %% of the rays hit something, nearest %.3f" % (args.depth, args.width, args.height, 100.0 * np.isfinite(depth).mean(), float(depth.min())))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
