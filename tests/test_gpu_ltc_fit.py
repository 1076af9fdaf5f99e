"""LTC tables fitted on the GPU (include/vkr_ltc_table.h fit_ltc_table, csrc/ltc_fit.hip) against their numpy restatement
(vulkan_renderer_amd/ltc_fit.py, pinned by tests/test_ltc_fit.py) in every bit of every float, the table they fill against
load_ltc_table() of the written files, and frames rendered with them against the CPU oracle in every bit."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import oracle_render
from vulkan_renderer_amd import capi, ltc_fit, renderer

pytestmark = pytest.mark.gpu

SEED = 515151
# interpreters that restate chains side by side (they do not touch the GPU)
PROCESSES = 8


@pytest.fixture(scope="module")
def device():
    r = renderer.Renderer()
    yield r
    r.close()


def host_tables(table):
    shape = (table.fresnel_count, table.inclination_count, table.roughness_count)
    return np.ctypeslib.as_array(table.host_rgba, shape + (4,)).copy(), np.ctypeslib.as_array(table.host_rg, shape + (2,)).copy()


def device_tables(r):
    """A read-back of device_rgba and device_rg of its own"""
    table = r.app.ltc_table
    shape = (table.fresnel_count, table.inclination_count, table.roughness_count)
    rgba, rg = np.zeros(shape + (4,), np.uint16), np.zeros(shape + (2,), np.uint16)
    r.sync()
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(rgba.ctypes.data), C.c_void_p(table.device_rgba), C.c_size_t(rgba.nbytes), 2) == 0
    assert hip.hipMemcpy(C.c_void_p(rg.ctypes.data), C.c_void_p(table.device_rg), C.c_size_t(rg.nbytes), 2) == 0
    return rgba, rg


def assert_same_bits(got, expected, what):
    differing = np.argwhere(got.view(np.uint32) != expected.view(np.uint32))
    assert len(differing) == 0, "%s: %d of %d floats differ, first at %s: %r against %r" % (
        what, len(differing), got.size, tuple(differing[0]), got[tuple(differing[0])], expected[tuple(differing[0])])


@pytest.mark.parametrize("R,F,N", [(8, 3, 16), (16, 2, 32), (8, 2, 128)])
def test_whole_tables_equal_the_restatement(device, R, F, N):
    device.fit_ltc_table(R, F, N)
    table = device.app.ltc_table
    assert (table.roughness_count, table.inclination_count, table.fresnel_count) == (R, R, F)
    got = device.ltc_fits()
    assert got.shape == (F, R, R, 5) and np.isfinite(got).all()
    assert_same_bits(got, ltc_fit.fit_table(R, F, N, 200, processes=PROCESSES), "table %dx%dx%d with %d^2 samples" % (R, R, F, N))
    rgba, rg = host_tables(table)
    expected_rgba, expected_rg = ltc_fit.quantize(got)
    assert np.array_equal(rgba, expected_rgba) and np.array_equal(rg, expected_rg)


def test_default_table_equals_the_restatement_on_six_chains(device, tmp_path):
    chains = [(0, 0), (2, 1), (5, 25), (16, 2), (31, 0), (31, 50)]
    milliseconds = device.fit_ltc_table()
    print("fit_ltc_table() of the default table: %.1f ms" % milliseconds)
    table = device.app.ltc_table
    assert (table.roughness_count, table.inclination_count, table.fresnel_count) == (32, 32, 51)
    got = device.ltc_fits()
    assert np.isfinite(got).all()
    expected = ltc_fit.fit_chains(chains, processes=PROCESSES)
    for x, i in chains:
        assert_same_bits(got[i, :, x], expected[(x, i)], "chain (%d, %d) of the default table" % (x, i))
    # the struct: host copies = device copies = what the loader makes of the written files, and the same constants
    rgba, rg = host_tables(table)
    device_rgba, device_rg = device_tables(device)
    assert np.array_equal(rgba, device_rgba) and np.array_equal(rg, device_rg)
    constants = bytes(table.constants)
    device.write_ltc_table(str(tmp_path / "fits"))
    loaded = capi.LtcTable()
    assert device.lib.load_ltc_table(C.byref(loaded), None, str(tmp_path / "fits").encode(), 51) == 0
    loaded_rgba, loaded_rg = host_tables(loaded)
    assert (loaded.roughness_count, loaded.inclination_count, loaded.fresnel_count) == (32, 32, 51)
    assert np.array_equal(rgba, loaded_rgba) and np.array_equal(rg, loaded_rg)
    assert bytes(loaded.constants) == constants
    device.lib.destroy_ltc_table(C.byref(loaded), None)
    raw = np.stack([np.fromfile(str(tmp_path / "fits" / ("fit%d.dat" % i)), np.float32, offset=8).reshape(32, 32, 5) for i in range(51)])
    assert_same_bits(raw, got, "the written files")


def test_a_second_fit_into_the_same_struct_gives_the_same_bytes_and_leaks_nothing(device):
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        device.sync()
        free, total = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    device.fit_ltc_table(8, 4, 16)
    first = (device.ltc_fits(),) + host_tables(device.app.ltc_table) + device_tables(device)
    before = free_bytes()
    for _ in range(3):
        device.fit_ltc_table(8, 4, 16)
    second = (device.ltc_fits(),) + host_tables(device.app.ltc_table) + device_tables(device)
    assert free_bytes() == before
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("settings", [(1, 51, 32, 200), (257, 51, 32, 200), (0, 51, 32, 200), (32, 1, 32, 200), (32, 257, 32, 200), (32, 0, 32, 200),
                                      (32, 51, 4, 200), (32, 51, 256, 200), (32, 51, 24, 200), (32, 51, 0, 200), (32, 51, 32, 0), None])
def test_refusals(device, capfd, settings):
    table = capi.LtcTable()
    table.fresnel_count = 7
    table.constants.roughness_factor = 2.0
    fits = C.POINTER(C.c_float)()
    # (the library prints through C's buffered stdout: what earlier calls left there goes first)
    C.CDLL(None).fflush(None)
    capfd.readouterr()
    if settings is None:
        # no device
        assert device.lib.fit_ltc_table(C.byref(table), C.byref(fits), None, None) == 1
    else:
        assert device.lib.fit_ltc_table(C.byref(table), C.byref(fits), C.byref(device.app.device), C.byref(capi.LtcFitSettings(*settings))) == 1
    C.CDLL(None).fflush(None)
    assert len(capfd.readouterr().out.strip().splitlines()) == 1
    assert bytes(table) == bytes(C.sizeof(capi.LtcTable)) and not fits


# ---- frames ----------------------------------------------------------------------------------------------------------

def make_renderer(dataset, config, width, height, frames_in_flight=1, **overrides):
    r = renderer.Renderer(frames_in_flight=frames_in_flight, arithmetic="libm")
    settings = dict(animate_noise=True, trace_shadow_rays=True, acceleration_structure="sah_device")
    settings.update(overrides)
    # (the visibility pass needs the acceleration structure, with or without shadow rays)
    renderer.setup_config(r, config, dataset, width=width, height=height, **settings)
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


def assert_frame_equals_the_oracle_frame_with_a_fitted_table(r, reads_table=True):
    synthetic_frame, _ = frame_and_oracle_frame(r)
    r.fit_ltc_table(16, 8, 16)
    table = r.app.ltc_table
    assert (table.roughness_count, table.fresnel_count) == (16, 8)
    inputs = r.host_inputs()
    rgba, rg = host_tables(table)
    assert np.array_equal(inputs["ltc_rgba"], rgba) and np.array_equal(inputs["ltc_rg"], rg)
    gpu, cpu = frame_and_oracle_frame(r)
    differing = int((gpu[..., :3].view(np.uint32) != cpu[..., :3].astype(np.float32).view(np.uint32)).any(axis=-1).sum())
    assert differing == 0, "%d pixels differ from the oracle's frame" % differing
    assert not np.isnan(gpu).any()
    # (diffuse_ggx_mis, the strategy of config 2, samples the GGX lobe itself and never looks into the table)
    assert np.array_equal(gpu, synthetic_frame) != reads_table


@pytest.mark.parametrize("config", [2, 3])
def test_frames_with_a_fitted_table_equal_the_oracle_frames(dataset, config):
    r = make_renderer(dataset, config, 160, 90, sample_count=2)
    assert_frame_equals_the_oracle_frame_with_a_fitted_table(r, reads_table=config == 3)
    r.close()


@pytest.mark.parametrize("frames_in_flight", [1, 3])
@pytest.mark.parametrize("trace_shadow_rays", [False, True])
@pytest.mark.parametrize("strategy", ["diffuse_specular_separately", "diffuse_specular_mis", "diffuse_specular_random"])
def test_every_strategy_that_reads_the_table_equals_the_oracle(dataset, strategy, trace_shadow_rays, frames_in_flight):
    r = make_renderer(dataset, 3, 128, 72, frames_in_flight=frames_in_flight, sample_count=1, sampling_strategies=strategy,
                      trace_shadow_rays=trace_shadow_rays)
    assert_frame_equals_the_oracle_frame_with_a_fitted_table(r)
    r.close()


def test_fits_do_not_outlive_their_table(dataset):
    """Renderer keeps the fits of fit_ltc_table() with their own size, and load_ltc_table() drops them"""
    r = renderer.Renderer()
    r.fit_ltc_table(8, 3, 8)
    assert r.ltc_fits().shape == (3, 8, 8, 5)
    r.lib.destroy_ltc_table(C.byref(r.app.ltc_table), C.byref(r.app.device))
    r.load_ltc_table(dataset["ltc"], dataset["fresnel_count"])
    with pytest.raises(RuntimeError):
        r.ltc_fits()
    with pytest.raises(RuntimeError):
        r.write_ltc_table("unused")
    r.close()


# ---- tools -------------------------------------------------------------------------------------------------------------

def test_convergence_takes_the_ltc_table_as_an_axis(capsys):
    """`convergence --ltc synthetic fitted` with the options that go with it, on a frame of 96x54"""
    import json
    from vulkan_renderer_amd import convergence
    capsys.readouterr()
    assert convergence.main(["--config", "3", "--frames", "4", "--reference-frames", "0", "--width", "96", "--height", "54", "--sample-count", "1",
                             "--strategy", "diffuse_specular_separately", "--ltc", "synthetic", "fitted", "--ltc-sample-count", "8", "--roughness-factor", "0.5"]) == 0
    lines = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert [line["ltc"] for line in lines] == ["synthetic", "fitted"]
    assert all("error" not in line and line["frames"] == 4 and line["mean_variance"] > 0 for line in lines)
    assert lines[0]["mean_variance"] != lines[1]["mean_variance"]
    # the default is the synthetic table, and the roughness factor reaches the frames
    capsys.readouterr()
    assert convergence.main(["--config", "3", "--frames", "4", "--reference-frames", "0", "--width", "96", "--height", "54", "--sample-count", "1",
                             "--strategy", "diffuse_specular_separately"]) == 0
    plain = [json.loads(line) for line in capsys.readouterr().out.splitlines() if line.startswith("{")]
    assert [line["ltc"] for line in plain] == ["synthetic"] and plain[0]["mean_variance"] != lines[0]["mean_variance"]


def test_experiments_render_with_a_fitted_table(tmp_path):
    """`experiments --ltc fitted`: the table is fitted instead of read from data/ggx_ltc_fit, which may then be absent"""
    from vulkan_renderer_amd import experiments
    root = str(tmp_path / "root")
    made = experiments.write_synthetic_data_root(root, grid=64, box_count=16)
    table = experiments.experiment_table()
    index = next(i for i in range(table.count) if table.experiments[i].screenshot_path == b"data/experiments/mis_plane_clamped_optimal_ours_2spp_%.3f.png")
    plain = experiments.run_experiment(index, root, frames=2, warmup=1, synthetic_inputs=True, fresnel_count=made["fresnel_count"], verbose=False)
    assert "ltc" not in plain
    before = open(plain["screenshot"], "rb").read()
    os.remove(plain["screenshot"])
    # (a link to the generated fits)
    os.remove(os.path.join(root, "data", "ggx_ltc_fit"))
    fitted = experiments.run_experiment(index, root, frames=2, warmup=1, synthetic_inputs=True, fresnel_count=made["fresnel_count"], verbose=False, ltc="fitted")
    assert fitted["ltc"] == "fitted" and open(fitted["screenshot"], "rb").read() != before
    with pytest.raises(RuntimeError):
        experiments.run_experiment(index, root, frames=2, warmup=1, synthetic_inputs=True, fresnel_count=made["fresnel_count"], verbose=False)
