"""Synthetic inputs of the frame filter (include/vkr_frame_filter.h), shared by tests/test_frame_filter.py (CPU: the numpy
restatement against independent statements, and the conditions that make each case mean something) and
tests/test_gpu_frame_filter.py (the kernels against the restatement).  Not collected by pytest.

The frame of every case is a valley seen from the origin: two planes z = 5 + 0.75 |X| that meet in a vertical crease (unit
normals (+-0.6, 0, 0.8): their cosine 0.28 underflows to 0 under the normal power), with
  - a band along the top whose normals are turned so that their cosine with the plane's is 0.7: 0.7^256 is a denormal;
  - a rectangle one unit nearer (a depth step without a change of the normal);
  - a rectangle where nothing is visible (sixteen zero bytes), and two more uncovered pixels: distance NaN and distance -1;
  - one pixel whose normal points away from every other;
  - a colour that is constant per patch, with Gaussian noise of a standard deviation per patch (0.05, 0.01 or 1e-4: the
    luminance weight of a quiet patch rejects its neighbours outright, t < -126) and that variance as the variance image.
Everything is scaled with the extent, so small frames keep what fits."""
import functools

import numpy as np

from vulkan_renderer_amd import frame_filter

f32 = np.float32
N1, N2 = np.array([0.6, 0.0, 0.8], f32), np.array([-0.6, 0.0, 0.8], f32)
# cos(phi) = 0.53125: dot(N1, N3) = 0.36 + 0.64 * 0.53125 = 0.7
N3 = np.array([0.6, 0.8 * np.sqrt(1.0 - 0.53125 ** 2), 0.8 * 0.53125], np.float64).astype(f32)
SETTINGS = dict(iteration_count=5, normal_squarings=8, sigma_luminance=4.0, sigma_depth=0.02, variance_scale=1.0)
SIGMAS = (0.05, 0.01, 1.0e-4)


def valley(width, height, seed, variance="true", modulation=False, non_finite=False):
    """-> dict of float32 images (height, width, 4): colour, variance (None for variance=None; zeros for "zero"), position,
    normal, modulation (or None), and clean (the colour without noise), plane (0: not covered, 1 / 2: the side of the
    crease) and special (the pixels named below)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:height, 0:width]
    crease = int(0.48 * width)
    X = ((xs - crease) * 0.1).astype(f32)
    Y = ((ys - height // 2) * 0.1).astype(f32)
    Z = (f32(5.0) + f32(0.75) * np.abs(X)).astype(f32)
    left = xs < crease
    normal = np.zeros((height, width, 4), f32)
    normal[..., :3] = np.where(left[..., None], N1, N2)
    band = (ys < max(1, int(0.13 * height))) & left
    normal[band, :3] = N3
    # the depth step
    step = (xs >= int(0.66 * width)) & (xs < int(0.85 * width)) & (ys >= int(0.22 * height)) & (ys < int(0.66 * height))
    Z = np.where(step, Z - f32(1.0), Z).astype(f32)
    position = np.stack([X, Y, Z, np.sqrt((X * X + Y * Y) + Z * Z)], axis=-1).astype(f32)
    normal[..., 3] = 0.5
    uncovered = (xs >= int(0.25 * width)) & (xs < max(int(0.25 * width) + 1, int(0.36 * width))) & (ys >= int(0.66 * height))
    special = {}
    if width >= 16 and height >= 16:
        special["nan_distance"], special["negative_distance"] = (height // 3, 2), (height // 3 + 2, 3)
        special["flipped_normal"] = (height // 2, int(0.1 * width))
        position[special["nan_distance"]][3] = np.nan
        position[special["negative_distance"]][3] = -1.0
        normal[special["flipped_normal"]][:3] = (0.0, 0.0, -1.0)
        uncovered[special["nan_distance"]] = uncovered[special["negative_distance"]] = True
    position[uncovered & ~np.isnan(position[..., 3]) & (position[..., 3] > 0)] = 0.0
    normal[uncovered & (position[..., 3] == 0)] = 0.0
    # the colour: constant per patch
    patch = max(2, min(width, height) // 4)
    columns, rows = (width + patch - 1) // patch, (height + patch - 1) // patch
    level = rng.uniform(0.1, 0.9, (rows, columns, 3)).astype(f32)
    sigma = np.array(SIGMAS, f32)[rng.integers(0, len(SIGMAS), (rows, columns))]
    clean = np.zeros((height, width, 4), f32)
    clean[..., :3] = level[ys // patch, xs // patch]
    clean[..., 3] = (xs + 0.5 * ys).astype(f32)
    sigma = np.broadcast_to(sigma[ys // patch, xs // patch][..., None], (height, width, 3))
    colour = clean.copy()
    images = {"clean": clean, "position": position, "normal": normal, "special": special, "variance": None, "modulation": None}
    if variance == "zero":
        images["variance"] = np.zeros((height, width, 4), f32)
        images["variance"][..., 3] = 1.0
    else:
        # (the channels of a pixel share their samples: one deviate for the three of them)
        colour[..., :3] += (sigma * rng.standard_normal((height, width, 1))).astype(f32)
        if variance == "true":
            images["variance"] = np.concatenate([(sigma * sigma).astype(f32), np.ones((height, width, 1), f32)], axis=-1)
    if modulation:
        m = rng.uniform(0.2, 1.0, (height, width, 4)).astype(f32)
        m[..., 3] = 0.25
        m[0, 0, :3] = (0.0, 1.0 / 512.0, -2.0)
        m[height - 1, width // 2, :3] = (1.0 / 256.0, 1.0e-30, 1.0)
        m[height // 2, width - 1, 1] = 0.0
        images["modulation"] = m
        # (what a renderer hands over: the radiance carries the albedo)
        colour[..., :3] *= np.maximum(m[..., :3], f32(1.0 / 256.0))
    if non_finite:
        # on the left of the crease: next to it, and in the open
        y = height // 2 + 3
        special.update(nan_at_crease=(y, crease - 1), inf_at_crease=(y + 2, crease - 1), nan_in_the_open=(height - 3, int(0.1 * width)),
                       inf_in_the_open=(5, int(0.3 * width)))
        colour[special["nan_at_crease"]][0] = np.nan
        colour[special["inf_at_crease"]][1] = np.inf
        colour[special["nan_in_the_open"]][2] = np.nan
        colour[special["inf_in_the_open"]][:3] = -np.inf
    images["colour"] = colour
    covered = position[..., 3] > 0
    images["plane"] = np.where(covered, np.where(left, 1, 2), 0)
    for name in ("colour", "variance", "position", "normal", "modulation", "clean"):
        if images[name] is not None:
            images[name].setflags(write=False)
    return images


# name -> (width, height, arguments of valley(), iteration count the case is made for)
CASES = {
    "83x45": (83, 45, dict(seed=1), 5),
    "16x16": (16, 16, dict(seed=2, modulation=True), 5),
    "7x3": (7, 3, dict(seed=3), 5),
    "33x35": (33, 35, dict(seed=4), 5),
    "zero_variance": (24, 20, dict(seed=5, variance="zero"), 5),
    "no_variance": (24, 20, dict(seed=6, variance=None), 5),
    "modulated": (24, 20, dict(seed=7, modulation=True), 5),
    "unmodulated": (24, 20, dict(seed=7), 5),
    "5x9_modulated": (5, 9, dict(seed=9, modulation=True), 5),
    "non_finite": (40, 24, dict(seed=8, non_finite=True), 5),
    "non_finite_no_variance": (40, 24, dict(seed=8, non_finite=True, variance=None), 5),
}
ITERATION_COUNTS = (1, 2, 5)


@functools.lru_cache(maxsize=None)
def inputs(name):
    width, height, arguments, _ = CASES[name]
    return valley(width, height, **arguments)


def settings(name, iteration_count=None):
    return dict(SETTINGS, iteration_count=iteration_count or CASES[name][3])


@functools.lru_cache(maxsize=None)
def expected(name, iteration_count):
    """-> (out_colour, out_variance or None, diagnostics per iteration) of the numpy restatement; computed once, left unchanged"""
    images = inputs(name)
    diagnostics = []
    out_colour, out_variance = frame_filter.filter_frame(images["colour"], images["variance"], images["position"], images["normal"], images["modulation"],
                                                         settings(name, iteration_count), diagnostics=diagnostics)
    for image in (out_colour, out_variance):
        if image is not None:
            image.setflags(write=False)
    return out_colour, out_variance, diagnostics


def assert_conditions(name):
    """What the case is there for, on the numpy side"""
    images = inputs(name)
    width, height, arguments, count = CASES[name]
    out_colour, out_variance, diagnostics = expected(name, count)
    covered = images["plane"] != 0
    assert covered.any() and len(diagnostics) == count
    assert out_colour[~covered].tobytes() == images["colour"][~covered].tobytes()
    assert out_colour[..., 3].tobytes() == images["colour"][..., 3].tobytes()
    if out_variance is not None:
        assert out_variance[~covered].tobytes() == images["variance"][~covered].tobytes() and (out_variance[covered][:, 3] == 1).all()
    if name == "83x45":
        assert width > 64 and height > 32 and width % 16 and height % 16
        assert (images["plane"] == 1).sum() > 500 and (images["plane"] == 2).sum() > 500 and (~covered).sum() > 100
        assert np.isnan(images["position"][images["special"]["nan_distance"]][3]) and not covered[images["special"]["nan_distance"]]
        assert not covered[images["special"]["negative_distance"]]
        for i, record in enumerate(diagnostics):
            # each of the four reasons to skip a tap, in every iteration
            for reason in ("out_of_frame", "uncovered", "exponent", "normal_weight"):
                assert record[reason] > 0, (i, reason, record)
            # the pixel whose normal points away keeps nothing but its centre
            assert record["centre_only"] >= 1, (i, record)
        assert sum(record["denormal_weights"] for record in diagnostics) > 0, diagnostics
        # taps at +-32 land inside the frame, outside it and on uncovered pixels
        assert 2 * 16 < width and 2 * 16 < height
    if name in ("16x16", "7x3", "5x9_modulated"):
        # no more than the tile of a workgroup
        assert width <= 16 and height <= 16
    if name == "5x9_modulated":
        assert images["modulation"] is not None and images["variance"] is not None
    if name == "7x3":
        # smaller than the footprint of step 1
        assert width < 5 or height < 5
        assert diagnostics[0]["out_of_frame"] > 0
    if name == "33x35":
        # step 16 reaches 32 pixels: the frame is barely wider, so that exactly the taps of its outermost pixels land inside
        assert count == 5 and 32 < width <= 35 and 32 < height <= 35
    if name == "zero_variance":
        assert not images["variance"][..., :3].any()
        # d_l = 1e-8: a neighbour of another patch is rejected outright
        assert all(record["exponent"] > 0 for record in diagnostics)
    if name in ("no_variance", "non_finite_no_variance"):
        assert images["variance"] is None and out_variance is None
    if name == "modulated":
        m = images["modulation"][..., :3]
        assert (m == 0).any() and ((m > 0) & (m < 1.0 / 256.0)).any() and (m < 0).any()
        plain = expected("unmodulated", count)[0]
        assert inputs("unmodulated")["modulation"] is None and plain.tobytes() != out_colour.tobytes()
    if name.startswith("non_finite"):
        special, colour = images["special"], images["colour"]
        assert not np.isfinite(colour[covered][:, :3]).all()
        for key in ("nan_at_crease", "inf_at_crease", "nan_in_the_open", "inf_in_the_open"):
            assert covered[special[key]] and not np.isfinite(colour[special[key]][:3]).all()
            assert images["plane"][special[key]] == 1
        # nothing crosses the crease: the other side of it is finite, next to the pixels and everywhere else
        across = images["plane"] == 2
        assert np.isfinite(out_colour[across][:, :3]).all()
        for key in ("nan_at_crease", "inf_at_crease"):
            y, x = special[key]
            assert across[y, x + 1] and not np.isfinite(out_colour[y, x, :3]).all()
        bad = ~np.isfinite(out_colour[..., :3]).all(axis=-1)
        if images["variance"] is None:
            # without a luminance weight they do spread, on their own side
            y, x = special["nan_at_crease"]
            assert np.isnan(out_colour[y, x - 1, 0]) and int(bad.sum()) > 4
        else:
            # the luminance weight rejects them: they stay where they are
            assert int(bad.sum()) == 4
