"""The restatement of the blue-noise dithered sampling table (vulkan_renderer_amd/noise_tables.py dithered_*, the rule of
include/vkr_noise_table.h generate_dithered_noise_table) against properties that do not come from it: the value set is a
net, the energy never rises and changes by exactly the accepted deltas, the pixels of a round cannot see each other, the
spectrum of the annealed array has little energy at low frequencies.  tests/test_gpu_dithered_noise.py pins the device
tables to it."""
import ctypes as C
import functools
import hashlib
import os
import re

import numpy as np
import pytest

from vulkan_renderer_amd import capi, renderer
from vulkan_renderer_amd import noise_tables as nt

SHAPES = ((16, 32), (32, 32), (64, 32))
SEEDS = (1, 0xC0FFEE11)
ROUND_COUNTS = (0, 256, 1024, 4096)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vkr_noise_table.h")


@functools.lru_cache(maxsize=None)
def annealed(width, height, seed):
    """Array 0 after each of ROUND_COUNTS, from one run: n rounds are the first n rounds of a longer run"""
    packed = nt.dithered_initial(width, height, seed, 0)
    arrays, done = {}, 0
    for rounds in ROUND_COUNTS:
        nt.dithered_rounds(packed, width, height, seed, 0, done, rounds - done)
        done = rounds
        arrays[rounds] = nt._dithered_unpack(packed.copy(), width, height)
    return arrays


# ---- symbols and host code -------------------------------------------------------------------------------------------

def test_the_library_declares_and_exports_the_dithered_generator():
    lib = capi.load()
    header = open(HEADER).read()
    for symbol, result in (("generate_dithered_noise_table", "int"), ("get_default_dithered_round_count", "uint32_t"), ("get_dithered_noise_weights", "void")):
        assert "VKR_API %s %s(" % (result, symbol) in header
        assert hasattr(lib, symbol) and symbol in capi.SIGNATURES
    assert int(re.search(r"#define VKR_DITHERED_ROUNDS_PER_LAUNCH (\d+)", header).group(1)) == nt.DITHERED_ROUNDS_PER_LAUNCH
    assert "blue_noise_dithered" in nt.GENERATED_TYPES and renderer.NOISE["blue_noise_dithered"] == nt.TYPES["blue_noise_dithered"] == 7
    assert nt.default_resolution("blue_noise_dithered") == (128, 128, 1)
    assert nt.file_name("blue_noise_dithered", (128, 128, 1)) == "data/noise/dithered_2d_rgba_128x128_01.blob"
    rounds = lib.get_default_dithered_round_count(capi.Extent3D(128, 128, 1))
    assert 0 < rounds <= min(1 << 20, nt.DITHERED_MAX_ROUNDS) and rounds & (rounds - 1) == 0


def test_the_weights_of_the_library_are_those_of_numpy():
    lib = capi.load()
    spatial, value = (C.c_uint32 * 169)(), (C.c_uint32 * 1449)()
    lib.get_dithered_noise_weights(spatial, value)
    expected_spatial, expected_value = nt.dithered_weights()
    assert expected_spatial.shape == (13, 13) and expected_value.shape == (1449,)
    assert np.array_equal(np.array(spatial[:], np.uint32), expected_spatial.ravel())
    assert np.array_equal(np.array(value[:], np.uint32), expected_value)
    # a product fits 32 bits; the weights fall with the distance; the centre does not count
    assert int(expected_spatial.max()) < 65536 and int(expected_value.max()) < 65536
    assert expected_spatial[6, 6] == 0 and expected_spatial[6, 7] == expected_spatial[5, 6] == round(65536 * np.exp(-1 / 2.1 ** 2))
    assert np.array_equal(expected_spatial, expected_spatial.T) and np.array_equal(expected_spatial, expected_spatial[::-1, ::-1])
    assert (np.diff(expected_value.astype(np.int64)) < 0).all()
    # the largest toroidal distance, (32768, 32768), is within the table
    assert int(nt._dithered_value_index(0, 0x80008000)) == 1448 and int(nt._dithered_value_index(5, 5)) == 0


def test_there_is_no_host_build_of_the_dithered_generator(capfd):
    lib = capi.load()
    # (the library prints through C's buffered stdout: what earlier calls left there goes first)
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    table = capi.NoiseTable()
    table.random_seed = 99
    table.resolution.width = 5
    assert lib.generate_dithered_noise_table(C.byref(table), None, capi.Extent3D(32, 32, 1), 0, 16) == 1
    assert bytes(table) == bytes(C.sizeof(capi.NoiseTable))
    C.CDLL(None).fflush(None)
    assert len(capfd.readouterr().out.strip().splitlines()) == 1


def test_the_distance_of_two_values_is_the_exact_integer_root():
    """r of the header against Python's integer square root, at the squares and next to them"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
    # pairs whose squared distance is k^2 - 1, k^2 and k^2 + 1: differences (k, 0) and (k, 1)
    k = np.arange(1, 32768, 37, dtype=np.uint32)
    a = np.concatenate([a, k, k | np.uint32(1 << 16), np.full(3, 0x80008000, np.uint32)])
    b = np.concatenate([b, np.zeros_like(k), np.zeros_like(k), np.array([0, 1, 0x10000], np.uint32)])
    import math
    for va, vb, got in zip(a.tolist(), b.tolist(), nt._dithered_value_index(a, b).tolist()):
        ax, ay = abs((va & 0xFFFF) - (vb & 0xFFFF)), abs((va >> 16) - (vb >> 16))
        ax, ay = min(ax, 65536 - ax), min(ay, 65536 - ay)
        assert got == math.isqrt(ax * ax + ay * ay) >> 5


def test_resolutions_and_round_counts_outside_the_range_are_refused():
    for resolution in ((8, 64, 1), (256, 256, 1), (512, 64, 1), (48, 48, 1), (32, 32, 3), (32, 32, 0), (16, 16, 1)):
        with pytest.raises(ValueError):
            nt.check_dithered_resolution(*resolution)
    with pytest.raises(ValueError):
        nt.check_dithered_resolution(32, 32, 1, (1 << 22) + 1)
    for resolution in ((16, 32, 1), (256, 128, 1), (128, 256, 2), (128, 128, 1)):
        nt.check_dithered_resolution(*resolution, 1 << 22)


# ---- the rule --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width,height", SHAPES)
def test_every_channel_is_a_permutation_before_and_after(width, height):
    n = width * height
    shift = 16 - (n.bit_length() - 1)
    for seed in SEEDS:
        values = nt.dithered_values(width, height, seed, 0)
        assert values.dtype == np.uint32 and values.shape == (n,)
        for rounds, array in annealed(width, height, seed).items():
            assert array.shape == (height, width, 2) and array.dtype == np.uint16
            for channel in range(2):
                assert np.array_equal(np.sort(array[..., channel].ravel().astype(np.int64) >> shift), np.arange(n)), (seed, rounds, channel)
            # and the array holds the value set itself
            assert np.array_equal(np.sort(nt._dithered_pack(array)), np.sort(values))
    # arrays and seeds differ
    assert not np.array_equal(nt.dithered_values(width, height, 1, 0), nt.dithered_values(width, height, 1, 1))
    assert not np.array_equal(nt.dithered_values(width, height, 1, 0), nt.dithered_values(width, height, 2, 0))
    assert np.array_equal(nt.dithered_array(width, height, 1, 0, 0), annealed(width, height, 1)[0])


@pytest.mark.parametrize("width,height", SHAPES)
def test_the_energy_never_rises_and_the_quality_measures_improve(width, height):
    """Measured on these shapes and seeds: the low-frequency share is 0.89 ... 1.15 before and 0.077 ... 0.092 after 3000
    rounds (bounds: > 0.5 and < 0.25, a factor of two off either), the neighbour distance rises from 0.381 ... 0.386 to
    0.430 ... 0.435 (0.3826 is the mean toroidal distance of independent values)."""
    for seed in SEEDS:
        arrays = annealed(width, height, seed)
        energies = [nt.dithered_energy(arrays[rounds]) for rounds in ROUND_COUNTS]
        shares = [nt.dithered_low_frequency_share(arrays[rounds]) for rounds in ROUND_COUNTS]
        distances = [nt.dithered_neighbour_distance(arrays[rounds]) for rounds in ROUND_COUNTS]
        print("%dx%d, seed %d: energies %s, low-frequency shares %s, neighbour distances %s" % (width, height, seed, energies, ["%.3f" % v for v in shares], ["%.4f" % v for v in distances]))
        assert all(later <= earlier for earlier, later in zip(energies, energies[1:]))
        assert energies[-1] < energies[0]
        assert shares[0] > 0.5 and shares[-1] < 0.25
        assert distances[-1] > distances[0]
        assert 0.36 < distances[0] < 0.41


def test_the_energy_changes_by_the_accepted_deltas():
    """16x32, 300 rounds: the total energy recomputed from scratch after every round"""
    width, height, seed = 16, 32, 7
    packed = nt.dithered_initial(width, height, seed, 1)
    energy = nt.dithered_energy(nt._dithered_unpack(packed, width, height))
    accepted = 0
    for k in range(300):
        deltas = []
        nt.dithered_rounds(packed, width, height, seed, 1, k, 1, deltas)
        assert len(deltas) == 1 and deltas[0] <= 0
        accepted += deltas[0] < 0
        after = nt.dithered_energy(nt._dithered_unpack(packed, width, height))
        assert after == energy + deltas[0], k
        energy = after
    assert 30 < accepted < 300


@pytest.mark.parametrize("width,height", SHAPES)
def test_the_pixels_of_a_round_are_more_than_6_apart(width, height):
    tile_count = (width // 16) * (height // 16)
    masks = set()
    for k in range(1000):
        pixels, mask = nt.dithered_round_pixels(width, height, 5, 3, k)
        assert pixels.shape == (tile_count,) and 1 <= mask <= tile_count - 1
        masks.add(mask)
        x, y = pixels % width, pixels // width
        dx, dy = np.abs(x[:, None] - x[None, :]), np.abs(y[:, None] - y[None, :])
        chebyshev = np.maximum(np.minimum(dx, width - dx), np.minimum(dy, height - dy))
        assert (chebyshev[~np.eye(tile_count, dtype=bool)] > 6).all(), k
    assert masks == set(range(1, tile_count))
    # the rounds differ and visit the whole image
    seen = np.zeros(width * height, bool)
    for k in range(1000):
        seen[nt.dithered_round_pixels(width, height, 5, 3, k)[0]] = True
    assert seen.mean() > 0.95


def test_the_table_holds_its_arrays_and_has_a_recorded_digest():
    table = nt.dithered_table(16, 32, 1, 1, 512)
    assert table.shape == (1, 32, 16, 4) and table.dtype == np.uint16
    assert np.array_equal(table[0, :, :, 0:2], nt.dithered_array(16, 32, 1, 0, 512))
    assert np.array_equal(table[0, :, :, 2:4], nt.dithered_array(16, 32, 1, 1, 512))
    assert np.array_equal(table, nt.table("blue_noise_dithered", (16, 32, 1), 1, 512))
    # recorded when the rule was written: a change of the rule shows here first
    assert hashlib.sha256(table.tobytes()).hexdigest() == "6a0291dcbc77cca1e68547c29a188cbd4de3e41b7b13e458ca274a60fd5beb46"
