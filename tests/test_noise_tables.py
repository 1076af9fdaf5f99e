"""The restatement of the generated noise tables (vulkan_renderer_amd/noise_tables.py, the rules of
include/vkr_noise_table.h) against properties that do not come from it: the net property of the Sobol blocks, values
written out from the recurrence, a toy integrand, a float64 re-check of the void-and-cluster ranks by FFT convolution
and the spectrum of the thresholded dither arrays.  tests/test_gpu_noise_tables.py pins the device tables to it."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

from vulkan_renderer_amd import capi, renderer
from vulkan_renderer_amd import noise_tables as nt

SOBOL_TYPES = ("sobol", "owen", "burley_owen")
SOBOL_SIZES = ((16, 2), (64, 8), (256, 64))


@functools.lru_cache(maxsize=None)
def sobol_table(noise_type, width, depth, seed):
    return nt.sobol_table(noise_type, width, depth, seed)


@functools.lru_cache(maxsize=None)
def blue_ranks(width, height, seed, a):
    return nt.blue_ranks(width, height, seed, a)


# ---- symbols ---------------------------------------------------------------------------------------------------------

def test_the_library_declares_and_exports_the_generator():
    lib = capi.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vkr_noise_table.h")).read()
    for symbol in ("generate_noise_table", "write_noise_table"):
        assert "VKR_API int %s(" % symbol in header
        assert hasattr(lib, symbol) and symbol in capi.SIGNATURES
    for name in nt.GENERATED_TYPES:
        assert renderer.NOISE[name] == nt.TYPES[name]
    assert [renderer.NOISE[n] for n in ("white", "blue", "ahmed", "sobol", "owen", "burley_owen", "blue_noise_dithered")] == [0, 1, 2, 4, 5, 6, 7]


def test_there_is_no_host_build_of_the_generator(capfd):
    """device == NULL is refused with one line and a zeroed struct, whatever the type"""
    lib = capi.load()
    # (the library prints through C's buffered stdout: what earlier calls left there goes first)
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    for noise_type in (1, 4, 5, 6):
        table = capi.NoiseTable()
        table.random_seed = 99
        table.resolution.width = 5
        assert lib.generate_noise_table(C.byref(table), None, capi.Extent3D(16, 16, 2), noise_type, 0) == 1
        assert bytes(table) == bytes(C.sizeof(capi.NoiseTable))
        C.CDLL(None).fflush(None)
        assert len(capfd.readouterr().out.strip().splitlines()) == 1


# ---- Sobol family ----------------------------------------------------------------------------------------------------

def test_direction_numbers_and_first_points_follow_the_recurrence():
    """Written out by hand from v[k] = v[k - s] ^ (v[k - s] >> s) ^ XOR a_j v[k - j]: m-values 1 3 5 15 17 (dimension 1),
    1 3 3 9 29 (dimension 2: m_k = 2 m_(k-1) ^ 4 m_(k-2) ^ m_(k-2)), 1 3 1 5 31 (dimension 3: m_k = 4 m_(k-2) ^ 8 m_(k-3) ^ m_(k-3))"""
    v = nt.direction_numbers()
    assert v.shape == (4, 32) and v.dtype == np.uint32
    expected_m = {0: [1, 1, 1, 1, 1], 1: [1, 3, 5, 15, 17], 2: [1, 3, 3, 9, 29], 3: [1, 3, 1, 5, 31]}
    for d, ms in expected_m.items():
        assert [int(v[d][k]) for k in range(5)] == [m << (31 - k) for k, m in enumerate(ms)], d
    # point i is the XOR of the v[k] of its set bits: in units of 1 / 8
    eighths = np.array([[0, 0, 0, 0], [4, 4, 4, 4], [2, 6, 6, 6], [6, 2, 2, 2], [1, 5, 3, 1], [5, 1, 7, 5], [3, 3, 5, 7], [7, 7, 1, 3]])
    assert np.array_equal(nt.sobol_points(0, 8).T, (eighths << 29).astype(np.uint32))
    # and the points do not depend on where a range starts
    assert np.array_equal(nt.sobol_points(5, 3), nt.sobol_points(0, 8)[:, 5:8])
    assert np.array_equal(nt.sobol_points((1 << 32) - 2, 2)[0], np.array([0x7FFFFFFF, 0xFFFFFFFF], np.uint32))


@pytest.mark.parametrize("width,depth", SOBOL_SIZES)
@pytest.mark.parametrize("noise_type", SOBOL_TYPES)
def test_every_block_fills_its_slice_exactly_once(noise_type, width, depth):
    # (checked here from the points themselves, not through sobol_table()'s own assertion)
    blocks = range(2 * depth) if width < 256 else (0, 1, 2, 63, 64, 127)
    for block in blocks:
        x, y, _, _ = nt.sobol_block(noise_type, width, 3, block)
        assert x.max() < width and y.max() < width
        counts = np.bincount(y.astype(np.int64) * width + x, minlength=width * width)
        assert counts.min() == 1 and counts.max() == 1, block
    table = sobol_table(noise_type, width, depth, 3)
    assert table.shape == (depth, width, width, 4) and table.dtype == np.uint16
    slices = [table[k, :, :, 2 * p:2 * p + 2].tobytes() for k in range(depth) for p in range(2)]
    assert len(set(slices)) == 2 * depth


def test_owen_scrambling_is_nested():
    """The first differing bit of two inputs is the first differing bit of their images: a permutation of every subtree"""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)
    # partners that agree with a in a random number of leading bits
    keep = rng.integers(0, 32, a.size)
    b = (a ^ (np.uint32(0x80000000) >> keep.astype(np.uint32))) ^ (rng.integers(0, 1 << 32, a.size, dtype=np.uint64).astype(np.uint32) >> (keep + 1).astype(np.uint32))
    for seed_d in (nt.dimension_seed(0, 0), nt.dimension_seed(77, 3)):
        sa, sb = nt.owen_scramble(a, seed_d), nt.owen_scramble(b, seed_d)

        def first_difference(p, q):
            return np.floor(np.log2((p ^ q).astype(np.float64))).astype(np.int64)
        assert np.array_equal(first_difference(a, b), 31 - keep)
        assert np.array_equal(first_difference(sa, sb), 31 - keep)
    # and it flips about half of the bits
    flipped = np.unpackbits((nt.owen_scramble(a, 1234) ^ a).view(np.uint8)).mean()
    assert 0.49 < flipped < 0.51
    # the bits a texel does not use are left out without changing the others
    assert np.array_equal(nt.owen_scramble(a, 99, 12), nt.owen_scramble(a, 99) & np.uint32(0xFFF00000))


def test_burley_scrambling_is_nested_too():
    rng = np.random.default_rng(6)
    a = rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)
    keep = rng.integers(0, 32, a.size)
    b = (a ^ (np.uint32(0x80000000) >> keep.astype(np.uint32))) ^ (rng.integers(0, 1 << 32, a.size, dtype=np.uint64).astype(np.uint32) >> (keep + 1).astype(np.uint32))
    sa, sb = nt.burley_scramble(a, 4242), nt.burley_scramble(b, 4242)
    assert np.array_equal(np.floor(np.log2((sa ^ sb).astype(np.float64))).astype(np.int64), 31 - keep)
    assert np.array_equal(nt.reverse_bits(np.array([1, 0x80000000, 0x00010000, 0xF0000001], np.uint32)), np.array([0x80000000, 1, 0x00008000, 0x8000000F], np.uint32))


@pytest.mark.parametrize("width,depth", SOBOL_SIZES[:2])
def test_seeds(width, depth):
    assert np.array_equal(sobol_table("sobol", width, depth, 3), nt.sobol_table("sobol", width, depth, 4))
    for noise_type in ("owen", "burley_owen"):
        assert not np.array_equal(sobol_table(noise_type, width, depth, 3), nt.sobol_table(noise_type, width, depth, 4))
        assert not np.array_equal(sobol_table(noise_type, width, depth, 3), sobol_table("sobol", width, depth, 3))
    assert not np.array_equal(sobol_table("owen", width, depth, 3), sobol_table("burley_owen", width, depth, 3))


def test_resolutions_outside_the_ranges_are_refused():
    for resolution in ((2, 2, 1), (8192, 8192, 1), (48, 48, 2), (64, 32, 2), (64, 64, 3), (4096, 4096, 256)):
        with pytest.raises(ValueError):
            nt.check_sobol_resolution(*resolution)
    assert nt.check_sobol_resolution(4096, 4096, 128) == 12
    for resolution in ((2, 16, 1), (256, 16, 1), (16, 24, 1), (16, 16, 6)):
        with pytest.raises(ValueError):
            nt.check_blue_resolution(*resolution)


def white_table(width, height, depth):
    """load_noise_table()'s white noise (host/noise_table.c)"""
    return (nt.wang(np.arange(width * height * depth * 4, dtype=np.uint32) + np.uint32(243708)) & np.uint32(0xFFFF)).astype(np.uint16).reshape(depth, height, width, 4)


def toy_mean_squared_errors(table, counts):
    """f(a, b) = exp(-3 ((a - 0.3)^2 + (b - 0.6)^2)) + [a b > 0.2].  The estimate of a pixel from n consecutive pairs that
    start at the even block 2 l0 (RG of layer l0, BA of layer l0, RG of layer l0 + 1, ...; layers wrap), its squared
    error against the integral averaged over pixels and l0"""
    depth, height, width, _ = table.shape
    u = (table.astype(np.float64) + 0.5) / 65536.0
    a, b = u[..., 0::2], u[..., 1::2]  # (D, H, W, pair)
    f = np.exp(-3.0 * ((a - 0.3) ** 2 + (b - 0.6) ** 2)) + (a * b > 0.2)
    # block order: (layer, pair) -> 2 layer + pair
    f = np.moveaxis(f, 3, 1).reshape(2 * depth, height, width)

    def gaussian(c):
        return 0.5 * math.sqrt(math.pi / 3.0) * (math.erf(math.sqrt(3.0) * (1.0 - c)) + math.erf(math.sqrt(3.0) * c))
    integral = gaussian(0.3) * gaussian(0.6) + 1.0 - 0.2 * (1.0 + math.log(5.0))
    errors = {}
    doubled = np.concatenate([f, f])
    sums = np.concatenate([np.zeros((1, height, width)), np.cumsum(doubled, axis=0)])
    for n in counts:
        starts = np.arange(0, 2 * depth, 2)
        estimates = (sums[starts + n] - sums[starts]) / n
        errors[n] = float(((estimates - integral) ** 2).mean())
    return errors


@pytest.mark.parametrize("noise_type", SOBOL_TYPES)
def test_toy_integrand_has_less_error_than_with_white_noise(noise_type):
    """At the default resolution of the type, 256x256x64, for every n = 2 ... 64.  Measured: the ratio to white noise falls
    from 0.57 ... 0.69 at n = 2 to 0.14 ... 0.35 at n = 64.  The resolution matters for the two points of a texel: in a
    64x64x64 table n = 2 has 1.07 (sobol) to 1.31 (burley_owen) of white noise's error and only n >= 3 is below it (the
    pair of a texel comes from two consecutive blocks, and which points of them share a texel depends on m); that table
    is printed, not asserted."""
    counts = tuple(range(2, 65))
    for width in (64, 256):
        white = toy_mean_squared_errors(white_table(width, width, 64), counts)
        ours = toy_mean_squared_errors(sobol_table(noise_type, width, 64, 11), counts)
        for n in (2, 3, 4, 8, 16, 32, 64):
            print("%s %dx%dx64, n = %d: mean squared error %.4g, white %.4g, ratio %.3f" % (noise_type, width, width, n, ours[n], white[n], ours[n] / white[n]))
    for n in counts:
        assert ours[n] < white[n], (n, ours[n], white[n])
    # (and white noise behaves like independent samples: the error halves with twice the samples)
    assert 0.4 < white[64] / white[32] < 0.6


# ---- blue noise ------------------------------------------------------------------------------------------------------

def test_blue_arrays_are_permutations_and_differ():
    for width, height, depth in ((16, 16, 2), (32, 8, 1), (8, 4, 2), (4, 4, 2)):
        table = nt.blue_table(width, height, depth, 5)
        assert table.shape == (depth, height, width, 4) and table.dtype == np.uint16
        n = width * height
        expected = ((np.arange(n) * 65536 + 32768) // n).astype(np.uint16)
        arrays = [table[k, :, :, c] for k in range(depth) for c in range(4)]
        for a, array in enumerate(arrays):
            assert np.array_equal(np.sort(array.ravel()), expected)
            assert np.array_equal(array, nt.blue_array(width, height, 5, a))
        # (4x4: n1 = 1, and the relaxation moves a single one to pixel 0 whatever the seed - one array, documented)
        assert len({array.tobytes() for array in arrays}) == (len(arrays) if n > 16 else 1)
        assert np.array_equal(arrays[0], nt.blue_array(width, height, 6, 0)) == (n == 16)
    ranks = blue_ranks(16, 16, 5, 0)
    assert np.array_equal(np.sort(ranks.ravel()), np.arange(256))


def energies_by_fft(pattern):
    height, width = pattern.shape
    dx = np.minimum(np.arange(width), width - np.arange(width)).astype(np.float64)
    dy = np.minimum(np.arange(height), height - np.arange(height)).astype(np.float64)
    kernel = np.exp(-(dx[None, :] ** 2 + dy[:, None] ** 2) / (2.0 * 1.5 * 1.5))
    return np.fft.irfft2(np.fft.rfft2(pattern.astype(np.float64)) * np.fft.rfft2(kernel), s=pattern.shape)


@pytest.mark.parametrize("size", [16, 32, 64])
def test_blue_ranks_hold_in_float64(size):
    """Independent of the float32 walk: for every 7th rank r the pixel of rank r is the tightest cluster of {rank <= r}
    (r < n1), the largest void of {rank < r} (n1 <= r < N / 2), the tightest cluster of {rank >= r} (r >= N / 2), within a
    relative energy gap of N 2^-23, the worst-case rounding of N float32 additions"""
    ranks = blue_ranks(size, size, 2, 1)
    n = size * size
    n1 = n // 10
    tolerance = n * 2.0 ** -23
    worst = 0.0
    for r in range(0, n, 7):
        pixel = ranks == r
        if r < n1:
            ones = ranks <= r
        elif r < n // 2:
            ones = ranks < r
        else:
            ones = ranks >= r
        energy = energies_by_fft(ones)
        if n1 <= r < n // 2:
            extreme = energy[~ones].min()
            gap = (energy[pixel][0] - extreme) / extreme
        else:
            extreme = energy[ones].max()
            gap = (extreme - energy[pixel][0]) / extreme
        worst = max(worst, gap)
        assert gap <= tolerance, (r, gap)
    print("%dx%d: largest relative energy gap %.3g (bound %.3g)" % (size, size, worst, tolerance))


def low_frequency_share(pattern):
    """Mean of P = |FFT2(pattern - mean)|^2 over radial frequencies 0 < r < 1 / 8, divided by the mean over r > 0"""
    height, width = pattern.shape
    power = np.abs(np.fft.fft2(pattern.astype(np.float64) - pattern.mean())) ** 2
    k, l = np.arange(width), np.arange(height)
    radius = np.hypot(np.minimum(k, width - k)[None, :] / width, np.minimum(l, height - l)[:, None] / height)
    return power[(radius > 0) & (radius < 0.125)].mean() / power[radius > 0].mean()


@pytest.mark.parametrize("size", [16, 32, 64])
def test_thresholded_blue_arrays_have_little_energy_at_low_frequencies(size):
    ranks = blue_ranks(size, size, 2, 1)
    n = size * size
    rng = np.random.default_rng(size)
    for threshold in (0.1, 0.25, 0.5, 0.75):
        share = low_frequency_share(ranks < threshold * n)
        white = low_frequency_share(rng.permutation(n).reshape(size, size) < threshold * n)
        print("%dx%d, threshold %.2f: low-frequency share %.4f (white noise %.3f)" % (size, size, threshold, share, white))
        assert share < 0.2, (threshold, share)


# ---- host plumbing ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise_type,resolution,name", [
    ("owen", (64, 64, 8), "data/noise/owen_2d_rgba_64x64_08.blob"),
    ("sobol", (16, 16, 2), "data/noise/sobol_2d_rgba_16x16_02.blob"),
    ("burley_owen", (16, 16, 2), "data/noise/burley_owen_2d_rgba_16x16_02.blob"),
    ("blue", (16, 8, 2), "data/noise/blue_noise_rgba_16x08_02.blob")])
def test_a_restated_table_is_read_back_by_load_noise_table(tmp_path, monkeypatch, noise_type, resolution, name):
    array = nt.table(noise_type, resolution, 9)
    path = nt.write_blob(array, noise_type, str(tmp_path))
    assert os.path.relpath(path, str(tmp_path)) == name and nt.file_name(noise_type, resolution) == name
    assert os.path.getsize(path) == array.nbytes
    monkeypatch.chdir(tmp_path)
    scene = renderer.HostScene()
    try:
        scene.load_noise_table(noise_type, resolution)
        table = scene.app.noise_table
        assert (table.resolution.width, table.resolution.height, table.resolution.depth) == resolution
        assert table.random_seed == nt.RANDOM_SEED and not table.device_data
        loaded = np.ctypeslib.as_array(table.host_data, array.shape)
        assert loaded.tobytes() == array.tobytes()
        # write_noise_table() writes the same file under the same name
        os.remove(path)
        assert scene.lib.write_noise_table(C.byref(table), renderer.NOISE[noise_type], None) == 0
        assert open(name, "rb").read() == array.tobytes()
        other = str(tmp_path / "elsewhere.blob")
        assert scene.lib.write_noise_table(C.byref(table), renderer.NOISE[noise_type], other.encode()) == 0
        assert open(other, "rb").read() == array.tobytes()
        # no file name for white noise, no data in an empty table
        assert scene.lib.write_noise_table(C.byref(table), 0, None) == 1
        assert scene.lib.write_noise_table(C.byref(capi.NoiseTable()), renderer.NOISE[noise_type], other.encode()) == 1
    finally:
        scene.close()
