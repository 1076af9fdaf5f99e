"""Noise tables generated on the GPU (include/vkr_noise_table.h generate_noise_table, csrc/noise_generators.hip) against
their numpy restatement (vulkan_renderer_amd/noise_tables.py, pinned by tests/test_noise_tables.py) in every byte, and
frames rendered with them against the CPU oracle in every bit."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import oracle_render
from vulkan_renderer_amd import capi, convergence, renderer
from vulkan_renderer_amd import noise_tables as nt

pytestmark = pytest.mark.gpu

SEED = 424242


@pytest.fixture(scope="module")
def device():
    r = renderer.Renderer()
    yield r
    r.close()


def host_table(r):
    n = r.app.noise_table.resolution
    return np.ctypeslib.as_array(r.app.noise_table.host_data, (n.depth, n.height, n.width, 4)).copy()


def device_table(r):
    """A read-back of device_data of its own"""
    n = r.app.noise_table.resolution
    out = np.zeros((n.depth, n.height, n.width, 4), np.uint16)
    r.sync()
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(r.app.noise_table.device_data), C.c_size_t(out.nbytes), 2) == 0
    return out


@pytest.mark.parametrize("width,depth", [(16, 2), (64, 8), (256, 64)])
@pytest.mark.parametrize("noise_type", ["sobol", "owen", "burley_owen"])
def test_sobol_family_equals_the_restatement(device, noise_type, width, depth):
    for seed in (0, 0xC0FFEE11):
        device.generate_noise_table(noise_type, (width, width, depth), seed)
        table = device.app.noise_table
        assert (table.resolution.width, table.resolution.height, table.resolution.depth) == (width, width, depth)
        assert table.random_seed == nt.RANDOM_SEED
        got = host_table(device)
        expected = nt.sobol_table(noise_type, width, depth, seed)
        differing = int((got != expected).sum())
        assert differing == 0, "%d of %d channels differ (seed %d)" % (differing, got.size, seed)
        assert np.array_equal(device_table(device), got)


@pytest.mark.parametrize("width,height,depth,arrays", [(16, 16, 64, None), (32, 32, 16, None), (64, 64, 64, (0, 1, 2, 3, 77, 130, 254, 255)),
                                                        (128, 128, 1, (1, 2)), (8, 32, 2, None), (4, 4, 1, None)])
def test_blue_noise_equals_the_restatement(device, width, height, depth, arrays):
    seed = 31 + width
    device.generate_noise_table("blue", (width, height, depth), seed)
    table = device.app.noise_table
    assert (table.resolution.width, table.resolution.height, table.resolution.depth) == (width, height, depth)
    assert table.random_seed == nt.RANDOM_SEED
    got = host_table(device)
    assert np.array_equal(device_table(device), got)
    for a in (range(4 * depth) if arrays is None else arrays):
        expected = nt.blue_array(width, height, seed, a)
        differing = int((got[a // 4, :, :, a % 4] != expected).sum())
        assert differing == 0, "array %d: %d of %d texels differ" % (a, differing, expected.size)
    # every array, compared or not, is a permutation of the ranks
    n = width * height
    ranks = ((np.arange(n) * 65536 + 32768) // n).astype(np.uint16)
    assert np.array_equal(np.sort(got.reshape(depth, n, 4), axis=1), np.broadcast_to(ranks[None, :, None], (depth, n, 4)))


def test_default_resolutions(device):
    device.generate_noise_table("blue")
    n = device.app.noise_table.resolution
    assert (n.width, n.height, n.depth) == (64, 64, 64)
    device.generate_noise_table("burley_owen", seed=5)
    n = device.app.noise_table.resolution
    assert (n.width, n.height, n.depth) == (256, 256, 64)
    assert np.array_equal(host_table(device)[:2], nt.sobol_table("burley_owen", 256, 2, 5))


@pytest.mark.parametrize("noise_type,resolution", [
    ("white", (64, 64, 8)), ("ahmed", (64, 64, 8)), ("blue_noise_dithered", (128, 128, 1)), (3, (64, 64, 8)), (8, (64, 64, 8)),
    # not powers of two
    ("owen", (48, 48, 4)), ("sobol", (64, 64, 6)), ("blue", (24, 16, 4)), ("blue", (16, 16, 3)),
    # out of range
    ("sobol", (2, 2, 4)), ("owen", (8192, 8192, 1)), ("burley_owen", (64, 32, 4)), ("blue", (2, 16, 1)), ("blue", (256, 64, 1)), ("blue", (64, 64, 0)), ("owen", (64, 64, 0)),
    # 2 D W H > 2^32
    ("sobol", (4096, 4096, 256)), ("owen", (1024, 1024, 4096))])
def test_refusals(device, capfd, noise_type, resolution):
    table = capi.NoiseTable()
    table.random_seed = 17
    table.resolution.depth = 3
    # (the library prints through C's buffered stdout: what earlier calls left there goes first)
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    assert device.lib.generate_noise_table(C.byref(table), C.byref(device.app.device), capi.Extent3D(*resolution), renderer._enum(renderer.NOISE, noise_type), 1) == 1
    C.CDLL(None).fflush(None)
    assert len(capfd.readouterr().out.strip().splitlines()) == 1
    assert bytes(table) == bytes(C.sizeof(capi.NoiseTable))


# ---- frames ----------------------------------------------------------------------------------------------------------

def make_renderer(dataset, config, width, height, frames_in_flight=1, **overrides):
    r = renderer.Renderer(frames_in_flight=frames_in_flight, arithmetic="libm")
    renderer.setup_config(r, config, dataset, width=width, height=height, animate_noise=True, trace_shadow_rays=True, acceleration_structure="sah_device", **overrides)
    r.create_targets()
    r.create_pass()
    r.render_visibility()
    return r


def frame_and_oracle_frame(r):
    r.app.noise_table.random_seed = SEED
    r.render()
    gpu = r.read_radiance()
    r.app.noise_table.random_seed = SEED
    cpu, _, _ = oracle_render(r, visibility=r.read_visibility(), math_mode=renderer.ORACLE_MATH_MODE["libm"])
    return gpu, cpu


@pytest.mark.parametrize("noise_type,resolution", [("blue", None), ("sobol", None), ("owen", (128, 128, 16)), ("burley_owen", (64, 64, 8)), ("blue", (32, 16, 4))])
@pytest.mark.parametrize("config", [2, 3])
def test_frames_with_generated_tables_equal_the_oracle_frames(dataset, config, noise_type, resolution):
    r = make_renderer(dataset, config, 160, 90, sample_count=2)
    white, _ = frame_and_oracle_frame(r)
    r.generate_noise_table(noise_type, resolution, 3)
    n = r.app.noise_table.resolution
    assert (n.width, n.height, n.depth) == (resolution or nt.default_resolution(noise_type))
    constants = r.host_inputs()["constants"].view(np.uint32)
    assert (constants[184 // 4], constants[188 // 4], constants[192 // 4]) == (n.width - 1, n.height - 1, n.depth - 1)
    gpu, cpu = frame_and_oracle_frame(r)
    differing = int((gpu[..., :3].view(np.uint32) != cpu[..., :3].astype(np.float32).view(np.uint32)).any(axis=-1).sum())
    assert differing == 0, "%d pixels differ from the oracle's frame" % differing
    assert not np.isnan(gpu).any() and not np.array_equal(gpu, white)
    r.close()


@pytest.mark.parametrize("noise_type,resolution", [("owen", (64, 64, 8)), ("blue", (16, 16, 4))])
def test_written_tables_load_to_the_same_bytes_and_the_same_frame(dataset, tmp_path, monkeypatch, noise_type, resolution):
    monkeypatch.chdir(tmp_path)
    r = make_renderer(dataset, 3, 160, 90, sample_count=2)
    r.generate_noise_table(noise_type, resolution, 8)
    generated = host_table(r)
    r.app.noise_table.random_seed = SEED
    r.render()
    frame = r.read_radiance()
    path = r.write_noise_table(noise_type, str(tmp_path))
    assert os.path.relpath(path, str(tmp_path)) == nt.file_name(noise_type, resolution)
    assert open(path, "rb").read() == generated.tobytes()
    r.finish_frames()
    r.lib.destroy_noise_table(C.byref(r.app.noise_table), C.byref(r.app.device))
    r.load_noise_table(noise_type, resolution)
    assert np.array_equal(host_table(r), generated) and np.array_equal(device_table(r), generated)
    r.app.noise_table.random_seed = SEED
    r.render()
    assert np.array_equal(r.read_radiance().view(np.uint32), frame.view(np.uint32))
    r.close()


@pytest.mark.parametrize("sample_count", [2, 8])
def test_owen_table_has_less_variance_than_white_noise(dataset, sample_count):
    """Config 3 at 256x256 with shadow rays, 64 frames of animated noise from a fixed seed, through convergence.measure().
    On the CPU oracle (256x144, 64 frames) the mean variance relative to white noise was 0.79 (sobol), 0.82 (owen),
    0.83 (burley_owen) and 0.98 (blue) at both sample counts."""
    r = make_renderer(dataset, 3, 256, 256, frames_in_flight=3, sample_count=sample_count)
    white = convergence.measure(r, 64, seed=1000)
    results = {}
    for noise_type in ("owen", "sobol", "burley_owen", "blue"):
        r.generate_noise_table(noise_type, seed=0)
        results[noise_type] = convergence.measure(r, 64, seed=1000)
        print("sample_count %d, %s: mean variance %.6g, white %.6g, ratio %.4f" % (sample_count, noise_type, results[noise_type]["mean_variance"], white["mean_variance"], results[noise_type]["mean_variance"] / white["mean_variance"]))
    r.close()
    assert white["mean_variance"] > 0
    assert results["owen"]["mean_variance"] < white["mean_variance"]
