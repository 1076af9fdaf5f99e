"""Inputs and a binary64 restatement of the material texture sampler, shared by tests/test_textures.py (the CPU oracle
against the restatement) and tests/test_gpu_texture_sampler.py (the device sampler against the oracle).  Not collected by
pytest.

The restatement is written from the rule in the sampler's comment (oracle/oracle.h, csrc/shading_inputs.h), not from its
code: N = min(ceil(P_max / P_min), 16, ceil(P_max)) trilinear taps at level log2(P_max / N), clamped to the chain, at
uv + (i / (N + 1) - 1 / 2) d(uv), i = 1 ... N, averaged; repeat addressing; sRGB texels decoded before filtering; a texel
coordinate that no int holds addresses texel 0.  It takes the float32 inputs as they are and computes in binary64."""
import functools

import numpy as np

MAX_TAPS = 16
SAMPLE_COUNT = 1 << 16

# (name, width, height, levels): 1-texel-wide levels, extents that are odd, not square and no power of two, chains that stop
# before 1x1 (48x20 has six levels, 8x8 four), a long chain and the texture of the rendered test frames
TEXTURES = [("1x1", 1, 1, 1), ("2x2", 2, 2, 2), ("4x4", 4, 4, 3), ("5x3", 5, 3, 3), ("64x1", 64, 1, 7), ("1x64", 1, 64, 7),
            ("48x20_3_levels", 48, 20, 3), ("8x8_2_levels", 8, 8, 2), ("256x16", 256, 16, 9), ("32x32", 32, 32, 6)]
TEXTURE_IDS = [t[0] for t in TEXTURES]


def level_extents(width, height, levels):
    extents = []
    for _ in range(levels):
        extents.append((width, height))
        width, height = max(width // 2, 1), max(height // 2, 1)
    return extents


@functools.lru_cache(maxsize=None)
def make_texture(name):
    """-> a dict as oracle.make_frame takes it ("srgb" 0: set it as needed).  Every level has random bytes of its own - a
    wrongly chosen texel or level shows - with 0 and 255 among them."""
    _, width, height, levels = TEXTURES[TEXTURE_IDS.index(name)]
    rng = np.random.default_rng(1000 + TEXTURE_IDS.index(name))
    chain = []
    for w, h in level_extents(width, height, levels):
        texels = rng.integers(0, 256, (h * w, 4), dtype=np.uint8)
        # (two channels only: the one texel of a 1x1 level keeps two random bytes, whose filtering is not exact in float32)
        texels[0, 0], texels[-1, 1] = 0, 255
        chain.append(texels)
    texels = np.concatenate(chain)
    texels.setflags(write=False)
    return {"texels": texels, "width": width, "height": height, "mip_count": levels, "srgb": 0}


def _next(x, direction):
    return np.nextafter(np.float32(x), np.float32(direction * np.inf))


def footprints_in_texels(width, height, levels):
    """-> (generic, rare): lists of (ax, ay, bx, by), the two screen-space derivatives in texels of level 0 (binary64; the
    inputs are these divided by the extents and rounded to float32).  rare: the footprints that sit on a discontinuity of the
    sampler on purpose - P_max / N an exact power of two or the float next to one (the level pair changes there), px == py (the
    tap count does) - of which make_inputs() takes few enough to leave the bounds on such disagreements intact."""
    generic, rare = [], []
    top = levels - 1
    # P_max / N: magnified, around 1, three values inside every level's binade up to 4x the coarsest level (top + 2: the clamp)
    rhos = [2.0 ** -6, 0.11, 0.73] + [2.0 ** l * f for l in range(top + 3) for f in (1.19, 1.5, 1.83)]
    powers = [float(v) for l in range(top + 3) for v in (2.0 ** l, _next(2.0 ** l, -1), _next(2.0 ** l, 1))]

    def add(out, p_max, p_min, angle, x_major):
        c, s = np.cos(angle), np.sin(angle)
        longer, shorter = (p_max * c, p_max * s), (-p_min * s, p_min * c)
        out.append(longer + shorter if x_major else shorter + longer)

    for taps in range(2, MAX_TAPS + 1):
        # P_max / P_min = taps - 1 / 2: in the middle between two steps of the ceiling
        for x_major in (True, False):
            for angle in (0.0, 0.6):  # along an axis of the texture, and diagonal
                for rho in rhos:
                    add(generic, rho * taps, rho * taps / (taps - 0.5), angle, x_major)
        for i, rho in enumerate(powers):
            add(rare, rho * taps, rho * taps / (taps - 0.5), 0.0, (taps + i) % 2 == 0)
    # one tap: a nearly round footprint of less than a texel (the ceiling of the quotient is 2, ceil(P_max) = 1 caps it) ...
    for rho in rhos[:3]:
        for angle in (0.0, 0.6):
            add(generic, rho, rho * 0.98, angle, angle == 0.0)
    # ... and, above one texel, ONLY the tie px == py.  P = width height 2^m: the derivatives P / width and P / height, their
    # products with the extents and the lengths are all exact in float32, so the tie holds in every arithmetic; m puts P into the
    # binade of each level, and beyond the chain.
    for l in range(top + 3):
        tie = width * height * 2.0 ** (l - int(np.floor(np.log2(width * height))))
        rare.append((tie, 0.0, 0.0, tie))
    # more stretched than the limit of 16
    for ratio in (17.0, 100.0, 1000.0):
        for x_major in (True, False):
            for angle in (0.0, 0.6):
                for rho in rhos:
                    add(generic, rho * MAX_TAPS, rho * MAX_TAPS / ratio, angle, x_major)
    return generic, rare


# derivatives that are zero, subnormal, so small that their square underflows, infinite, NaN
SPECIAL_DERIVATIVES = [0.0, -0.0, 1.0e-45, -5.0e-39, 1.0e-20, np.inf, -np.inf, np.nan]


def special_footprints(width, height):
    """-> (n, 4) float32 derivatives (du/dx, dv/dx, du/dy, dv/dy) with special values on one axis and on both"""
    normal = [(0.37 / width, 0.0), (2.9 / width, 1.1 / height), (0.0, 9.3 / height)]
    out = []
    for s in SPECIAL_DERIVATIVES:
        for n in normal:
            out += [(s, 0.0) + n, (0.0, s) + n, (s, s) + n, n + (s, 0.0), n + (0.0, s), n + (s, s), (s, 0.5 * n[1]) + n, n + (0.5 * n[0], s)]
        for t in SPECIAL_DERIVATIVES:
            out += [(s, 0.0, 0.0, t), (s, s, t, t), (0.0, s, t, 0.0)]
    return np.array(out, np.float32)


def structured_coordinates(width, height):
    """-> (n, 2) float32 texture coordinates where addressing goes wrong"""
    f32 = np.float32
    us, vs = [], []
    for extent, out in ((width, us), (height, vs)):
        texels = sorted({0, 1, extent // 2, extent - 1})
        out += [(i + 0.5) / extent for i in texels]  # texel centres: u * extent - 1 / 2 is an integer
        out += [i / extent for i in texels + [extent]]  # texel edges, the seam at 0 and 1
        out += [float(k) for k in (-1, 2, 7)]  # the seam, whole turns away
        out += [_next(1.0, -1), _next(1.0, 1), _next(0.0, 1), -_next(0.0, 1), 0.5 / extent - 1.0, -0.25 / extent, -3.0 - 1.5 / extent, -0.3]
        out += [1.0e3, -1.0e3, 1.0e6 + 0.37, -1.0e6]
        for bound in (2.0 ** 24, 2.0 ** 31):  # |u * extent| on either side of 2^24 (no fraction left) and of 2^31 (no int left)
            edge = f32(bound / extent)
            out += [sign * value for sign in (1.0, -1.0) for value in (edge, _next(edge, -1), _next(edge, 1), _next(_next(edge, 1), 1))]
        out += [np.inf, -np.inf, np.nan]
    n = max(len(us), len(vs))
    # every special u with an ordinary v, every special v with an ordinary u, and the specials with each other
    pairs = [(u, 0.3 + 0.01 * i) for i, u in enumerate(us)] + [(0.6 - 0.01 * i, v) for i, v in enumerate(vs)]
    pairs += [(us[i % len(us)], vs[(i * 7 + 3) % len(vs)]) for i in range(2 * n)]
    return np.array(pairs, f32)


@functools.lru_cache(maxsize=None)
def make_inputs(name):
    """-> (SAMPLE_COUNT, 6) float32: uv, duv_dx, duv_dy for the texture `name`.  Every footprint meets structured coordinates and
    coordinates from the workload's range, [0, 8] x [-7, 1]."""
    _, width, height, levels = TEXTURES[TEXTURE_IDS.index(name)]
    rng = np.random.default_rng(77 + TEXTURE_IDS.index(name))
    generic, rare = footprints_in_texels(width, height, levels)
    scale = np.array([width, height, width, height], np.float64)
    # (the special derivatives at half the weight of the others: a NaN or a zero makes P_max / P_min exactly 1 or puts it on
    # another step of the tap count more often than not, and the share of such inputs is bounded)
    generic = (np.array(generic) / scale).astype(np.float32)
    generic = np.concatenate([generic, generic, special_footprints(width, height)])
    rare = (np.array(rare) / scale).astype(np.float32)
    # the rare ones twice each (one structured and one random coordinate), the others share the rest evenly
    rare_count = 2 * len(rare)
    assert rare_count < SAMPLE_COUNT // 64
    index = np.arange(SAMPLE_COUNT - rare_count)
    derivatives = np.concatenate([generic[index % len(generic)], rare, rare])
    turn = np.concatenate([index // len(generic), np.zeros(len(rare), np.int64), np.ones(len(rare), np.int64)])
    which = np.concatenate([index % len(generic), np.arange(len(rare)), np.arange(len(rare))])
    structured = structured_coordinates(width, height)
    uv = (rng.random((SAMPLE_COUNT, 2)) * 8.0 + np.array([0.0, -7.0])).astype(np.float32)
    use_structured = turn % 2 == 0
    uv[use_structured] = structured[(turn // 2 * 5 + which * 3)[use_structured] % len(structured)]
    inputs = np.concatenate([uv, derivatives], axis=1).astype(np.float32)
    inputs.setflags(write=False)
    return inputs


# ---- the restatement --------------------------------------------------------------------------------------------------------

def glsl_max(x, y):
    """max() as the GLSL specification words it: y if x < y, otherwise x (a NaN y is ignored, a NaN x returned)"""
    return np.where(x < y, y, x)


def glsl_min(x, y):
    return np.where(y < x, y, x)


def footprint(width, height, levels, inputs):
    """What the rule makes of the derivatives: -> dict of taps (int), l0, l1 (int), fraction, x_major, tap_steps.  tap_steps: the
    tap count changes when the two quotients it is the ceiling of move by 1e-3 of themselves."""
    d = np.asarray(inputs, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        px, py = np.sqrt((d[:, 2] * width) ** 2 + (d[:, 3] * height) ** 2), np.sqrt((d[:, 4] * width) ** 2 + (d[:, 5] * height) ** 2)
        x_major = px >= py
        p_max, p_min = glsl_max(px, py), np.where(x_major, py, px)

        def tap_count(ratio, length):
            taps = glsl_min(glsl_min(np.ceil(ratio), float(MAX_TAPS)), glsl_max(np.ceil(length), 1.0))
            return np.where(taps >= 1.0, taps, 1.0)
        taps = tap_count(p_max / p_min, p_max)
        tap_steps = np.zeros(len(d), bool)
        for a in (1.0 - 1.0e-3, 1.0 + 1.0e-3):
            for b in (1.0 - 1.0e-3, 1.0 + 1.0e-3):
                tap_steps |= tap_count(p_max / p_min * a, p_max * b) != taps
        rho = p_max / taps
        level = np.where(rho > 1.0, glsl_min(np.log2(np.where(rho > 1.0, rho, 1.0)), float(levels - 1)), 0.0)
    l0 = np.floor(level)
    return {"taps": taps.astype(np.int64), "l0": l0.astype(np.int64), "l1": np.minimum(l0 + 1, levels - 1).astype(np.int64),
            "fraction": level - l0, "x_major": x_major, "tap_steps": tap_steps}


def srgb_to_linear(v):
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


def restate(texture, inputs):
    """-> (samples (n, 2, 4) binary64: [:, 0] for a linear texture, [:, 1] for an sRGB one, footprint(...))"""
    width, height, levels = texture["width"], texture["height"], texture["mip_count"]
    extents = np.array(level_extents(width, height, levels), np.int64)
    first = np.concatenate([[0], np.cumsum(extents[:, 0] * extents[:, 1])[:-1]])
    bytes_ = np.asarray(texture["texels"], np.uint8).reshape(-1, 4)
    linear = bytes_ / 255.0
    values = np.stack([linear, np.concatenate([srgb_to_linear(linear[:, :3]), linear[:, 3:]], axis=1)], axis=1)  # (texels, 2, 4)
    d = np.asarray(inputs, np.float32).astype(np.float64)
    f = footprint(width, height, levels, inputs)
    du, dv = np.where(f["x_major"], d[:, 2], d[:, 4]), np.where(f["x_major"], d[:, 3], d[:, 5])

    def index(x0):
        inside = (x0 >= -2.0 ** 31) & (x0 < 2.0 ** 31)
        return np.where(inside, x0, 0.0).astype(np.int64)

    def bilinear(level, u, v):
        w, h, base = extents[level, 0], extents[level, 1], first[level]
        with np.errstate(all="ignore"):
            x, y = u * w - 0.5, v * h - 0.5
            x0, y0 = np.floor(x), np.floor(y)
            fx, fy = (x - x0)[:, None, None], (y - y0)[:, None, None]
        ix, iy = index(x0), index(y0)
        texel = lambda i, j: values[base + (j % h) * w + i % w]
        with np.errstate(all="ignore"):
            return (texel(ix, iy) * (1 - fx) + texel(ix + 1, iy) * fx) * (1 - fy) + (texel(ix, iy + 1) * (1 - fx) + texel(ix + 1, iy + 1) * fx) * fy

    total = np.zeros((len(d), 2, 4))
    for i in range(1, MAX_TAPS + 1):
        rows = np.nonzero(f["taps"] >= i)[0]
        if not len(rows):
            break
        taps = f["taps"][rows]
        with np.errstate(all="ignore"):
            offset = i / (taps + 1.0) - 0.5
            # (one tap: at uv itself, whatever the derivatives are)
            u = np.where(taps > 1, d[rows, 0] + du[rows] * offset, d[rows, 0])
            v = np.where(taps > 1, d[rows, 1] + dv[rows] * offset, d[rows, 1])
            fraction = f["fraction"][rows][:, None, None]
            total[rows] += bilinear(f["l0"][rows], u, v) * (1 - fraction) + bilinear(f["l1"][rows], u, v) * fraction
    return total / f["taps"][:, None, None], f


@functools.lru_cache(maxsize=None)
def restated(name):
    """restate() of make_texture(name) on make_inputs(name), computed once per session"""
    return restate(make_texture(name), make_inputs(name))


def finite_coordinates(inputs):
    return np.isfinite(inputs[:, :2]).all(axis=1)


@functools.lru_cache(maxsize=None)
def assert_coverage(name):
    """The inputs of a texture make the sampler take every tap count at every level the texture has, the clamp at the top of
    the chain and both major axes - by the restatement's count, at finite coordinates"""
    texture, inputs = make_texture(name), make_inputs(name)
    f = restated(name)[1]
    finite = finite_coordinates(inputs)
    pairs = set(zip(f["taps"][finite].tolist(), f["l0"][finite].tolist()))
    assert pairs >= {(taps, level) for taps in range(1, MAX_TAPS + 1) for level in range(texture["mip_count"])}
    assert ((f["l0"] == f["l1"]) & finite).sum() > 1000
    assert 0.4 < f["x_major"][finite].mean() < 0.6


def tolerance(texture, inputs):
    """What float32 may cost the sampler against binary64, absolute, per sample: 2^-21 (4 + |u| w + |v| h).  The float32 texel
    coordinate is off by at most one ulp of |u| w; that moves a bilinear weight by as much, between texels that differ by at
    most 1; about 30 rounded operations on values in [0, 1] come on top."""
    uv = np.abs(np.asarray(inputs, np.float32)[:, :2].astype(np.float64))
    return 2.0 ** -21 * (4.0 + uv[:, 0] * texture["width"] + uv[:, 1] * texture["height"])


def same_bits(a, b):
    """Bit for bit, NaN equals NaN: -> per row"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all(axis=-1)


# ---- a rendered frame that makes the sampler work: material textures that are not square, no powers of two and whose chains
# stop at 6x2 (five of seven levels), seen from a camera 12 cm above the ground plane that looks along it ----

GRAZING_DATASET = dict(grid=48, box_count=12, seed=1234, ltc_resolution=16, fresnel_count=8, textured=True, texture_size=(96, 40), texture_levels=5)
GRAZING_CAMERA = dict(position=(-3.0, -2.0, 0.12), rotation_x=0.49 * np.pi)
GRAZING_EXTENT = (96, 64)


def apply_grazing_case(scene, case, dataset):
    """golden_cases.apply_case at GRAZING_EXTENT with the grazing camera"""
    import golden_cases
    from vulkan_renderer_amd import synthetic
    golden_cases.apply_case(scene, case, dataset, *GRAZING_EXTENT)
    cam = synthetic.DEFAULT_CAMERA
    scene.set_camera(GRAZING_CAMERA["position"], GRAZING_CAMERA["rotation_x"], cam["rotation_z"], cam["vertical_fov"], cam["near"], cam["far"])


def assert_frame_works_the_sampler(frame, textures):
    """The texture reads of the frame reach a level >= 3 and 16 taps (at once, too), by the restatement's count"""
    import oracle
    inputs = oracle.texture_sampler_inputs(frame).reshape(-1, 6)
    inputs = inputs[~np.isnan(inputs[:, 0])]
    width, height, levels = GRAZING_DATASET["texture_size"] + (GRAZING_DATASET["texture_levels"],)
    assert all((t["width"], t["height"], t["mip_count"]) == (width, height, levels) for t in textures)
    f = footprint(width, height, levels, inputs)
    assert len(inputs) > 2000 and (f["l0"] >= 3).sum() >= 16 and (f["taps"] == MAX_TAPS).sum() >= 16
    assert ((f["l0"] >= 3) & (f["taps"] == MAX_TAPS)).sum() >= 16
    assert set(f["taps"].tolist()) == set(range(1, MAX_TAPS + 1))
