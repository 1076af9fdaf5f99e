"""Moving geometry (include/vkr_scene_update.h): the codes of the vertex positions, the numpy restatement of the refit
of csrc/bvh_refit.hip, a deterministic motion, and the smallest end-to-end use,

    python -m vulkan_renderer_amd.scene_update DATASET --frames N --amplitude A --out DIR [--policy refit|rebuild|auto] [--time]

which renders config 3 of a dataset directory of synthetic.write_dataset() while its mesh wobbles, one PNG per frame
through the device encoder.

The restatement works on the arrays that Renderer.read_acceleration_structure() returns.  Up to the fp32 boxes of the
leaves it is float32 with one rounding per operation, like the kernels; everything behind them is a minimum or a maximum
of 15-bit integers.  Its answers are therefore the kernels' bytes, whatever order the kernels' lanes arrive in."""
import argparse
import os
import sys

import numpy as np

from . import ray_queries

# scene_update_policy_t
POLICY = {"refit": 0, "rebuild": 1, "auto": 2}
CODE_MAX = (1 << 21) - 1
# csrc/lbvh.h
LEAF_BIT, WIDE_EMPTY, WIDE_EMPTY_BOX = 0x80000000, 0xFFFFFFFF, 0x00007FFF
GRID_MAX, GRID_MARGIN = np.float32(32767.0), np.float32(0.05)

_F = np.float32


# ---- codes ------------------------------------------------------------------------------------------------------------

def pack_positions(codes):
    """(..., 3) codes of 21 bits -> (n, 2) uint32, the two words per vertex of a scene file (include/vkr_scene.h)"""
    q = np.asarray(codes, np.uint32).reshape(-1, 3)
    if q.size and int(q.max()) > CODE_MAX:
        raise ValueError("a position code exceeds 21 bits")
    words = np.zeros((len(q), 2), np.uint32)
    words[:, 0] = q[:, 0] | ((q[:, 1] & 0x7FF) << 21)
    words[:, 1] = (q[:, 1] >> 11) | (q[:, 2] << 10)
    return words


def unpack_positions(words):
    """(n, 2) uint32 words -> (n, 3) uint32 codes: the inverse of pack_positions()"""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1, 2)
    return np.stack([w[:, 0] & 0x1FFFFF, ((w[:, 0] & 0xFFE00000) >> 21) | ((w[:, 1] & 0x3FF) << 11), (w[:, 1] & 0x7FFFFC00) >> 10], -1)


def quantize(positions, factor, summand):
    """The inverse of the de-quantisation code * factor + summand, rounded to the nearest code.
    -> (codes (..., 3) uint32, clamped (...) bool: vertices outside the de-quantisation box - the cells of the codes 0 ...
    2^21 - 1, half a cell around each - by more than a quarter of a cell, which were moved onto it.  (A quarter of a cell
    is what the float32 rounding of factor and summand can shift the far end of the box by: 2^21 cells times 2^-23.)"""
    p = np.asarray(positions, np.float64)
    q = (p - np.asarray(summand, np.float32).astype(np.float64)) / np.asarray(factor, np.float32).astype(np.float64)
    clamped = ((q < -0.75) | (q > CODE_MAX + 0.75)).any(axis=-1)
    return np.clip(np.rint(q), 0, CODE_MAX).astype(np.uint32), clamped


def padding(factor, summand):
    """The padding of the boxes of a mesh, float32 (make_build_params of csrc/bvh_build.hip)"""
    factor, summand = np.asarray(factor, _F), np.asarray(summand, _F)
    width = _F(2097152.0) * factor
    extent = max(float(np.abs(width).max()), float(np.abs(summand).max()), float(np.abs(summand + width).max()))
    return _F(2.0e-6) * _F(extent)


# ---- leaf boxes (step 1) -------------------------------------------------------------------------------------------------

def _fma32(a, b, c):
    """fmaf for float32 scalars: the product is exact in float64, the sum is rounded to odd there, so that the rounding to
    float32 is the only one that matters"""
    p = np.float64(a) * np.float64(b)
    c = np.float64(c)
    s = p + c
    t = s - p
    error = (p - (s - t)) + (c - t)
    if error != 0 and np.isfinite(s) and (int(np.float64(s).view(np.uint64)) & 1) == 0:
        s = np.nextafter(s, np.inf if error > 0 else -np.inf)
    return _F(s)


def slab_box(v, lo, hi, axis, j, count):
    """fragment_bounds() of csrc/bvh_leaf_boxes.h: the box of the part of triangle v (3, 3) float32, whose box is [lo, hi],
    inside slab j of count along `axis` -> (lo (3,), hi (3,)) float32"""
    v, lo, hi = np.asarray(v, _F), np.asarray(lo, _F), np.asarray(hi, _F)
    a0, a1 = lo[axis], hi[axis]
    s0 = a0 if j == 0 else _fma32(_F(j) / _F(count), a1 - a0, a0)
    s1 = a1 if j + 1 == count else _fma32(_F(j + 1) / _F(count), a1 - a0, a0)
    points = [[_F(x) for x in vertex] for vertex in v]
    for plane, sign in ((s0, _F(1)), (s1, _F(-1))):
        kept = []
        for i, p in enumerate(points):
            q = points[(i + 1) % len(points)]
            di, dj = sign * (p[axis] - plane), sign * (q[axis] - plane)
            if di >= 0:
                kept.append(p)
            if (di >= 0) != (dj >= 0):
                w = di / (di - dj)
                cut = [_fma32(w, q[k] - p[k], p[k]) for k in range(3)]
                cut[axis] = plane
                kept.append(cut)
        points = kept
    flo, fhi = np.full(3, 3.0e38, _F), np.full(3, -3.0e38, _F)
    for p in points:
        flo, fhi = np.minimum(flo, np.array(p, _F)), np.maximum(fhi, np.array(p, _F))
    if not flo[0] <= fhi[0]:
        flo, fhi = lo.copy(), lo.copy()
    return np.maximum(flo, lo), np.minimum(fhi, hi)


def longest_axis(lo, hi):
    e = np.asarray(hi, _F) - np.asarray(lo, _F)
    return 0 if (e[0] >= e[1] and e[0] >= e[2]) else (1 if e[1] >= e[2] else 2)


def leaf_boxes(tree, words, factor, summand):
    """-> (vertices (L, 3, 3) float32 of the triangles of the leaf slots, boxes (L, 6) float32: lo.xyz, hi.xyz, unpadded)
    for the position words of a mesh: the triangle's box, or where the build has split the triangle (leaf_fragments)
    the box of slab j of count along the longest axis of the triangle's new box"""
    primitive = np.ascontiguousarray(tree["triangle_vertices"][0::3, 3]).view(np.uint32)
    vertices = ray_queries.dequantize(words, factor, summand)[primitive]
    lo, hi = vertices.min(axis=1), vertices.max(axis=1)
    fragments = np.asarray(tree["leaf_fragments"], np.uint32)
    for slot in np.nonzero((fragments & 0xFFFF) > 1)[0]:
        j, count = int(fragments[slot] >> 16), int(fragments[slot] & 0xFFFF)
        lo[slot], hi[slot] = slab_box(vertices[slot], lo[slot].copy(), hi[slot].copy(), longest_axis(lo[slot], hi[slot]), j, count)
    return vertices, np.concatenate([lo, hi], -1)


# ---- the grid and the two trees (steps 2 to 5) ---------------------------------------------------------------------------

def choose_grid(lo, hi):
    """grid_origin, grid_inverse_cell for a padded root box, float32 (vkr_choose_bvh_grid of csrc/bvh_build.hip)"""
    lo, hi = np.asarray(lo, _F), np.asarray(hi, _F)
    cell = np.maximum(hi - lo, _F(1.0e-20)) / (GRID_MAX - _F(2.0))
    return lo - cell, _F(1.0) / cell


def quantize_boxes(boxes, pad, origin, inverse_cell):
    """(L, 6) float32 boxes -> (L, 3) uint32 packed lo | hi << 16 on the grid, padded and rounded outwards (quantize_box_axis)"""
    boxes = np.asarray(boxes, _F)
    q0 = np.floor((boxes[:, :3] - pad - origin) * inverse_cell - GRID_MARGIN)
    q1 = np.ceil((boxes[:, 3:] + pad - origin) * inverse_cell + GRID_MARGIN)
    q0, q1 = np.clip(q0, _F(0), GRID_MAX), np.clip(q1, _F(0), GRID_MAX)
    return q0.astype(np.uint32) | (q1.astype(np.uint32) << 16)


def merge_packed(a, b):
    """union of packed boxes: the minimum of the low halves, the maximum of the high halves"""
    return np.minimum(a & 0xFFFF, b & 0xFFFF) | (np.maximum(a >> 16, b >> 16) << 16)


def binary_children(nodes, inner):
    """-> (left, right) of the inner nodes `inner` of the threaded binary tree"""
    left = inner + 1
    link = nodes[left, 3]
    return left, np.where(link & LEAF_BIT, inner + 2, link).astype(np.int64)


def binary_levels(nodes):
    """the inner nodes of the binary tree, level by level from the root"""
    levels, frontier = [], np.zeros(1, np.int64)
    while True:
        inner = frontier[(nodes[frontier, 3] & LEAF_BIT) == 0]
        if not len(inner):
            return levels
        levels.append(inner)
        frontier = np.concatenate(binary_children(nodes, inner))


def tree_cost(nodes, grid_inverse_cell):
    """-> (the three integer sums of ex ey, ey ez, ez ex over the inner nodes, the cost of include/vkr_scene_update.h)"""
    inner = nodes[(nodes[:, 3] & LEAF_BIT) == 0].astype(np.uint64)
    e = (inner[:, :3] >> np.uint64(16)) - (inner[:, :3] & np.uint64(0xFFFF))
    sums = [int((e[:, a] * e[:, b]).sum(dtype=np.uint64)) for a, b in ((0, 1), (1, 2), (2, 0))]
    cell = 1.0 / np.asarray(grid_inverse_cell, np.float32).astype(np.float64)
    cost = float(np.float64(sums[0]) * (cell[0] * cell[1]) + np.float64(sums[1]) * (cell[1] * cell[2]) + np.float64(sums[2]) * (cell[2] * cell[0]))
    return sums, cost


def refit_reference(tree, words, factor, summand):
    """What update_scene_geometry() with scene_update_refit makes of the tree `tree` (Renderer.read_acceleration_structure())
    for the position words `words`: a dict with nodes, wide_nodes, triangle_vertices, grid_origin, grid_inverse_cell as
    in `tree`, and cost_sums, cost"""
    factor, summand = np.asarray(factor, _F), np.asarray(summand, _F)
    pad = padding(factor, summand)
    vertices, boxes = leaf_boxes(tree, words, factor, summand)
    out = {}
    triangles = tree["triangle_vertices"].copy()
    triangles[:, :3] = vertices.reshape(-1, 3)
    out["triangle_vertices"] = triangles
    # the grid from the padded box of the mesh
    origin, inverse_cell = choose_grid(boxes[:, :3].min(axis=0) - pad, boxes[:, 3:].max(axis=0) + pad)
    out["grid_origin"], out["grid_inverse_cell"] = origin, inverse_cell
    # binary tree: leaves from their boxes, inner nodes from their children, deepest level first
    nodes = tree["nodes"].copy()
    is_leaf = (nodes[:, 3] & LEAF_BIT) != 0
    leaf_node = np.zeros(len(boxes), np.int64)
    leaf_node[nodes[is_leaf, 3] & ~np.uint32(LEAF_BIT)] = np.nonzero(is_leaf)[0]
    nodes[leaf_node, :3] = quantize_boxes(boxes, pad, origin, inverse_cell)
    for inner in reversed(binary_levels(nodes)):
        left, right = binary_children(nodes, inner)
        nodes[inner, :3] = merge_packed(nodes[left, :3], nodes[right, :3])
    out["nodes"] = nodes
    # wide tree: lanes that name leaves from the leaf boxes, lanes that name inner nodes from the union of that node's lanes
    wide = None
    if tree["wide_nodes"] is not None:
        wide = tree["wide_nodes"].copy()
        links = wide[:, 12:16]
        present, names_leaf = links != WIDE_EMPTY, (links != WIDE_EMPTY) & ((links & LEAF_BIT) != 0)
        node_index, lane = np.nonzero(names_leaf)
        leaf_box = nodes[leaf_node[links[node_index, lane] & ~np.uint32(LEAF_BIT)], :3]
        for axis in range(3):
            wide[node_index, 4 * axis + lane] = leaf_box[:, axis]
        # the node and the lane that name every inner node
        parent, parent_lane = np.zeros(len(wide), np.int64), np.zeros(len(wide), np.int64)
        node_index, lane = np.nonzero(present & ~names_leaf)
        parent[links[node_index, lane]], parent_lane[links[node_index, lane]] = node_index, lane
        levels, frontier = [], np.zeros(1, np.int64)
        while len(frontier):
            levels.append(frontier)
            children = links[frontier]
            frontier = children[(children != WIDE_EMPTY) & ((children & LEAF_BIT) == 0)].astype(np.int64)
        for level in reversed(levels[1:]):
            for axis in range(3):
                lanes = wide[level, 4 * axis:4 * axis + 4]
                lo = np.where(present[level], lanes & 0xFFFF, 0xFFFF).min(axis=1)
                hi = np.where(present[level], lanes >> 16, 0).max(axis=1)
                wide[parent[level], 4 * axis + parent_lane[level]] = (lo | (hi << 16)).astype(np.uint32)
    out["wide_nodes"] = wide
    out["cost_sums"], out["cost"] = tree_cost(nodes, inverse_cell)
    return out


def differences(tree, expected):
    """-> the names among nodes, wide_nodes, triangle_vertices, grid_origin, grid_inverse_cell whose bytes differ"""
    names = []
    for name in ("nodes", "wide_nodes", "triangle_vertices", "grid_origin", "grid_inverse_cell"):
        a, b = tree[name], expected[name]
        if (a is None) != (b is None) or (a is not None and (a.shape != b.shape or a.tobytes() != b.tobytes())):
            names.append(name)
    return names


# ---- a motion ------------------------------------------------------------------------------------------------------------

def wobble(positions, t, amplitude=0.05, fixed=None, wavelength=4.0):
    """A deterministic displacement: every triangle of positions (T, 3, 3) moves as a whole along a small Lissajous
    figure of the given amplitude (world units); t = 0 is NOT the rest position.  The phase is that of a wave of the
    given length that runs through the scene, so that neighbours move together like the parts of a swaying object;
    wavelength None: a phase per triangle index, neighbours unrelated - a mesh shaken to pieces, the worst a refit
    can meet.  fixed: bool (T,), triangles that stay.  The result is clipped to the box of `positions`, so a mesh
    whose de-quantisation box is its own box never leaves it."""
    p = np.asarray(positions, np.float64)
    if wavelength is None:
        phase = (np.arange(len(p)) * 0.6180339887498949) % 1.0 * (2.0 * np.pi)
    else:
        phase = p.mean(axis=1) @ np.array([0.62, 0.54, 0.57]) * (2.0 * np.pi / wavelength)
    d = amplitude * np.stack([np.sin(t + phase), np.cos(1.3 * t + 2.0 * phase), np.sin(0.7 * t + 3.0 * phase)], -1)
    if fixed is not None:
        d[np.asarray(fixed, bool)] = 0.0
    flat = p.reshape(-1, 3)
    return np.clip(p + d[:, None, :], flat.min(axis=0), flat.max(axis=0))


class Wobble:
    """The motion of the command lines: the mesh of a Renderer as it is now - at rest -, and the position words of frame
    0, 1, ... of its wobble.  rest_words: what update_geometry() takes to put the mesh back."""

    def __init__(self, scene, amplitude):
        mesh = scene.app.scene.mesh
        self.amplitude = amplitude
        self.factor, self.summand = np.array(mesh.dequantization_factor[:], np.float32), np.array(mesh.dequantization_summand[:], np.float32)
        self.rest_words = np.ctypeslib.as_array(mesh.host_positions, (3 * mesh.triangle_count, 2)).copy()
        self.rest = ray_queries.dequantize(self.rest_words, self.factor, self.summand).astype(np.float64)

    def words(self, frame):
        codes, _ = quantize(wobble(self.rest, 0.5 * frame, self.amplitude), self.factor, self.summand)
        return pack_positions(codes)


# ---- command line ----------------------------------------------------------------------------------------------------------

def main(argv=None):
    parser = argparse.ArgumentParser(description="Renders config 3 of a dataset directory while its mesh wobbles: one PNG per frame.")
    parser.add_argument("dataset", help="a directory written by synthetic.write_dataset(): scene.vks, textures/, ltc/")
    parser.add_argument("--frames", type=int, default=8)
    parser.add_argument("--amplitude", type=float, default=0.05, help="of the wobble, in world units")
    parser.add_argument("--out", required=True, help="directory of the PNG files")
    parser.add_argument("--policy", choices=sorted(POLICY), default="refit")
    parser.add_argument("--rebuild-above", type=float, default=0.0)
    parser.add_argument("--width", type=int, default=640)
    parser.add_argument("--height", type=int, default=360)
    parser.add_argument("--time", action="store_true", help="print refit and rebuild milliseconds and the cost ratio per frame")
    args = parser.parse_args(argv)
    from . import renderer
    ltc = os.path.join(args.dataset, "ltc")
    dataset = {"scene": os.path.join(args.dataset, "scene.vks"), "textures": os.path.join(args.dataset, "textures"), "ltc": ltc,
               "fresnel_count": len([name for name in os.listdir(ltc) if name.startswith("fit")])}
    os.makedirs(args.out, exist_ok=True)
    r = renderer.Renderer()
    # (--time: a second copy of the scene that is rebuilt for every frame, so that the rendered one goes on being refitted)
    timer = renderer.Renderer() if args.time else None
    try:
        if timer:
            timer.load_scene(dataset["scene"], dataset["textures"], acceleration_structure=True)
        renderer.setup_config(r, 3, dataset, width=args.width, height=args.height)
        r.create_targets()
        r.create_pass()
        motion = Wobble(r, args.amplitude)
        for frame in range(args.frames):
            moved = motion.words(frame)
            report = r.update_geometry(moved, policy=args.policy, measure_cost=args.time, rebuild_above=args.rebuild_above)
            if args.time:
                line = "frame %d: %s %.3f ms, cost ratio %.4f" % (frame, "rebuild" if report["rebuilt"] else "refit", report["milliseconds"], report["cost"] / report["built_cost"] if report["built_cost"] else 0.0)
                print(line + ", a rebuild %.3f ms" % timer.update_geometry(moved, policy="rebuild")["milliseconds"])
            r.render_visibility()
            r.render()
            with open(os.path.join(args.out, "frame_%04d.png" % frame), "wb") as f:
                f.write(r.read_png())
    finally:
        r.close()
        if timer:
            timer.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
