"""Prepared polygons that are kept while the inputs of the launches stand still (csrc/kept_polygons.h "Prepared polygons
that are still true", csrc/prepared_polygons.hip): the first launch of an arrangement
prepares its polygons itself (plain), the second one also writes them to device memory (storing), and the launches after
it read them from there instead of preparing them (loading) - until any input of the preparation changes.  A loaded
polygon is the polygon, so every frame must be the frame of a pass that never keeps anything
(VKR_PREPARED_POLYGONS_MIB=0), in every bit: no tolerance anywhere.

Every test renders its sequence twice, each time with a renderer of its own that starts from the same noise seed: with
the cache (the default) and without.

The frame is 64 x 48 pixels of the benchmark scene from the benchmark camera: ground, boxes and sky, so that the 8x8
patches (one wave each) mix pixels that shade with pixels that do not (asserted below).  The lights (LIGHTS) are PLACED
for the ways through the preparation; which of them a frame really holds is asserted only where a frame can tell from
outside (test_the_frame_holds_what_the_lights_are_placed_for), the rest is the geometry of the placement:
  above     a quad over the ground in front of the camera, facing down: below it the central case, far to the side the
            decentral one; V = 5 without the clipped vertex
  triangle  three vertices in a pass whose polygons have room for five; alone, or with "low", a pass with V = 4, whose
            storing and loading kernels lay their words out differently (a quad of words there holds slots of both tables)
  standing  a quad that stands upright THROUGH the ground plane: the ground's horizon cuts it (three to five vertices), the
            pixels on its far side are behind its plane (side < 0), and next to it the specular polygon - clipped in the
            space of the LTC, whose horizon is tilted toward the reflection - can be culled while the diffuse one is not
  below     a quad far under the ground: below the horizon of every pixel whose normal points up - ground and tops of
            boxes, most of the frame; nothing is prepared there and the status word alone is stored.  Asserted: alone it
            leaves every shaded pixel of the frame black.  (Walls of boxes that face it prepare its polygons and find their
            rays blocked by the ground, which a frame cannot tell from a polygon that is clipped away.)
  low       a triangle that the ground plane cuts"""
import math

import numpy as np
import pytest

from helpers import DeviceBuffer
from vulkan_renderer_amd import renderer, synthetic

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT = 64, 48
QUAD = synthetic.QUAD
LIGHTS = {
    "above": synthetic.light_spec(QUAD, (-1.8, -0.2, 1.4), (math.pi, 0.0, 0.3), (6, 6, 8), (1.0, 0.8)),
    "triangle": synthetic.light_spec([(0, 0), (1, 0), (0, 1)], (-0.5, 1.5, 1.2), (0.8 * math.pi, 0.2, 0.9), (7, 6, 5), (1.2, 1.2)),
    "standing": synthetic.light_spec(QUAD, (-1.2, 0.6, -0.35), (0.5 * math.pi, 0.0, 0.5), (8, 6, 6), (1.4, 1.0)),
    "below": synthetic.light_spec(QUAD, (-1.0, 1.0, -6.0), (0.0, 0.0, 0.0), (9, 9, 9), (2.0, 2.0)),
    "low": synthetic.light_spec([(0, 0), (1, 0), (0.5, 1)], (-1.4, 0.4, -0.3), (0.5 * math.pi, 0.0, 2.0), (6, 8, 6), (1.5, 1.2)),
}
# ("triangles": no light has four vertices, so the pass is built for V = 4)
LIGHT_SETS = {"one": ["standing"], "two": ["above", "standing"], "four": ["above", "triangle", "standing", "below"], "triangles": ["triangle", "low"],
              "below": ["below"]}
QUADS_PER_PAIR = {"one": 16, "two": 16, "four": 16, "below": 16, "triangles": 13}
STRATEGIES = {"mis_clamped": ("diffuse_specular_mis", "optimal_clamped"), "mis_optimal": ("diffuse_specular_mis", "optimal"),
              "separately": ("diffuse_specular_separately", "balance")}
OFF = "0"


def start(dataset, lights="four", strategy="mis_clamped", frames_in_flight=1, width=WIDTH, height=HEIGHT, arithmetic=None):
    r = renderer.Renderer(frames_in_flight=frames_in_flight, arithmetic=arithmetic)
    strategies, heuristic = STRATEGIES[strategy]
    renderer.setup_config(r, 3, dataset, width=width, height=height, acceleration_structure="sah_device",
                          sampling_strategies=strategies, mis_heuristic=heuristic, animate_noise=True)
    r.set_lights([LIGHTS[name] for name in LIGHT_SETS[lights]])
    r.create_targets()
    return r


def sequences(monkeypatch, begin, steps, budgets=(None, OFF)):
    """One frame per entry of `steps` (a callable that changes an input before the frame, or None), once per budget (None: the
    default) -> per budget a list of {"image", "stats"}.  The noise is animated: frame k of either run draws the same numbers."""
    out = []
    for budget in budgets:
        if budget is None:
            monkeypatch.delenv("VKR_PREPARED_POLYGONS_MIB", raising=False)
        else:
            monkeypatch.setenv("VKR_PREPARED_POLYGONS_MIB", budget)
        r = begin()
        try:
            r.app.noise_table.random_seed = 4711
            r.create_pass()
            r.render_visibility()
            frames = []
            for step in steps:
                if step is not None:
                    step(r)
                r.render()
                # (read_radiance waits for the frame: a storing launch has completed when the next frame is planned)
                frames.append({"image": r.read_radiance(), "stats": r.prepared_polygon_statistics()})
            out.append(frames)
        finally:
            r.close()
            monkeypatch.delenv("VKR_PREPARED_POLYGONS_MIB", raising=False)
    return out


def modes(frames):
    return [f["stats"]["mode"] for f in frames]


def assert_frames_equal(warm, cold):
    assert len(warm) == len(cold)
    for index, (w, c) in enumerate(zip(warm, cold)):
        a, b = w["image"].view(np.uint32), c["image"].view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (index, w["stats"]["mode"], int((a != b).any(axis=-1).sum()))
    # animated noise: the frames of a sequence differ from each other, or equal frames would say nothing
    assert not np.array_equal(cold[0]["image"], cold[1]["image"])


def assert_never_kept(cold):
    for frame in cold:
        assert frame["stats"]["mode"] == "plain" and frame["stats"]["buffer_bytes"] == 0 and frame["stats"]["launches"]["storing"] == 0, frame["stats"]


@pytest.mark.parametrize("lights", ["one", "two", "four", "triangles"])
@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
def test_five_frames_standing_still(big_dataset, monkeypatch, strategy, lights):
    """plain, storing, loading, loading, loading - and every frame is the frame of a pass that keeps nothing"""
    warm, cold = sequences(monkeypatch, lambda: start(big_dataset, lights, strategy), [None] * 5)
    assert modes(warm) == ["plain", "storing", "loading", "loading", "loading"]
    assert_never_kept(cold)
    assert_frames_equal(warm, cold)
    # [light][quad][thread]: 16 quads of 16 bytes at V = 5 (62 words), 13 at V = 4 (52 words); one launch of 16 blocks of 256 threads
    assert warm[-1]["stats"]["buffer_bytes"] == len(LIGHT_SETS[lights]) * QUADS_PER_PAIR[lights] * 16 * 4096
    image = cold[0]["image"]
    assert 0.02 < (image[..., :3] == 0.0).all(axis=-1).mean() < 0.98, "the frame should hold lit pixels and sky or unlit ones"


@pytest.mark.parametrize("lights", ["four", "triangles"])
def test_polynomial_arithmetic(big_dataset, monkeypatch, lights):
    """the "exact" mode has storing and loading kernels of its own (the fast mode has none: next test)"""
    warm, cold = sequences(monkeypatch, lambda: start(big_dataset, lights, arithmetic="exact"), [None] * 4)
    assert modes(warm) == ["plain", "storing", "loading", "loading"]
    assert_never_kept(cold)
    assert_frames_equal(warm, cold)


def test_fast_arithmetic_keeps_nothing(big_dataset, monkeypatch):
    """no such kernels in the fast mode (its compiler may fuse a product of the preparation into a sum of the sampling):
    every launch is plain and nothing is allocated"""
    warm, cold = sequences(monkeypatch, lambda: start(big_dataset, arithmetic="fast"), [None] * 3)
    assert_never_kept(warm)
    assert_frames_equal(warm, cold)


def test_the_frame_holds_what_the_lights_are_placed_for(big_dataset):
    """(the premises of the docstring above that can be checked from outside: sky and geometry in the frame, and waves
    that mix them)"""
    r = start(big_dataset)
    try:
        r.create_pass()
        r.render_visibility()
        sky = r.read_visibility() == 0xFFFFFFFF
    finally:
        r.close()
    assert 0.02 < sky.mean() < 0.9
    patches = sky.reshape(HEIGHT // 8, 8, WIDTH // 8, 8).mean(axis=(1, 3))
    assert ((patches > 0.0) & (patches < 1.0)).any(), "no 8x8 patch mixes sky and geometry"
    # the light under the ground alone reaches no pixel: for the ground and the tops of the boxes its diffuse polygon is
    # clipped away, and the status word is all that is kept of the pair
    r = start(big_dataset, "below")
    try:
        r.create_pass()
        r.render_visibility()
        r.render()
        black = (r.read_radiance()[..., :3] == 0.0).all(axis=-1)
    finally:
        r.close()
    assert (~sky).mean() > 0.3 and black.all(), "the light under the ground should leave the whole frame black"


def moved_vertex(r):
    lights = [dict(LIGHTS[name]) for name in LIGHT_SETS["four"]]
    v = np.array(lights[1]["vertices_plane_space"], np.float32)
    v[2, 1] += 0.25
    lights[1]["vertices_plane_space"] = v
    r.set_lights(lights)


def other_radiance(r):
    lights = [dict(LIGHTS[name]) for name in LIGHT_SETS["four"]]
    lights[2]["radiant_flux"] = (3.0, 9.0, 4.0)
    r.set_lights(lights)


def nudged_camera(r):
    cam = synthetic.DEFAULT_CAMERA
    r.set_camera((cam["position"][0] + 1.0e-3, cam["position"][1], cam["position"][2]), cam["rotation_x"], cam["rotation_z"], cam["vertical_fov"], cam["near"], cam["far"])


def uploaded_visibility(r):
    r.upload_visibility(r.read_visibility())


def reloaded_ltc_table(dataset):
    def step(r):
        # the same fits into (most likely) the same allocations: only the table's upload serial tells
        r.sync()
        r.lib.destroy_ltc_table(renderer.C.byref(r.app.ltc_table), r._dev())
        r.load_ltc_table(dataset["ltc"], dataset["fresnel_count"])
    return step


def other_size(r):
    r.sync()
    r.set_settings(width=80, height=HEIGHT)
    r.create_targets()
    r.render_visibility()


def other_strategy(r):
    # (another kernel variant: the pass is created anew, as the reference recompiles its shader)
    r.sync()
    r.set_settings(sampling_strategies="diffuse_specular_separately")
    r.create_pass()


def fewer_lights(r):
    r.sync()
    r.set_lights([LIGHTS[name] for name in LIGHT_SETS["four"][:3]])
    r.create_pass()


@pytest.mark.parametrize("what", ["camera", "light_vertex", "light_radiance", "visibility_upload", "ltc_table", "frame_size", "strategy", "light_count"])
def test_one_input_changes(big_dataset, monkeypatch, what):
    """Three frames, ONE input changes, three frames: the launch after the change is plain, the next one stores, the third
    loads again - and all of them are the frames of a pass that keeps nothing."""
    change = {"camera": nudged_camera, "light_vertex": moved_vertex, "light_radiance": other_radiance, "visibility_upload": uploaded_visibility,
              "ltc_table": reloaded_ltc_table(big_dataset), "frame_size": other_size, "strategy": other_strategy, "light_count": fewer_lights}[what]
    warm, cold = sequences(monkeypatch, lambda: start(big_dataset), [None] * 3 + [change] + [None] * 2)
    assert modes(warm) == ["plain", "storing", "loading"] * 2
    assert_never_kept(cold)
    assert_frames_equal(warm, cold)


def test_three_frames_in_flight(big_dataset, monkeypatch):
    """Frames of 640 x 368 are submitted without a wait in between, each into a target of its own, until one of them has
    loaded while others were in flight and two more have followed it.  The first is plain, the second stores, and each of
    the others loads only if the storing launch was seen complete when it was planned or runs on the same stream, behind it
    (a launch on another stream that found it incomplete ran plain and was counted).  What tells from outside that no launch loaded too early: a launch that loads before the polygons
    are stored samples from whatever the buffer holds, and EVERY frame must be the frame of a pass that keeps nothing."""
    width, height = 640, 368
    results = []
    count = None
    for budget in (None, OFF):
        if budget is None:
            monkeypatch.delenv("VKR_PREPARED_POLYGONS_MIB", raising=False)
        else:
            monkeypatch.setenv("VKR_PREPARED_POLYGONS_MIB", budget)
        r = start(big_dataset, frames_in_flight=3, width=width, height=height)
        targets = []
        try:
            r.app.noise_table.random_seed = 4711
            r.create_pass()
            r.render_visibility()
            stats = []
            first_loading = None
            while len(stats) < (count if count is not None else 200):
                targets.append(DeviceBuffer(16 * (width + 64) * (height + 64)))
                r.render(targets[-1].ptr.value)
                stats.append(r.prepared_polygon_statistics())
                # (a launch on another stream than the storing launch's - frame 2's; the streams take turns - that loads)
                if first_loading is None and stats[-1]["mode"] == "loading" and (len(stats) - 1) % 3 != 1:
                    first_loading = len(stats) - 1
                if count is None and first_loading is not None and len(stats) >= max(first_loading + 3, 6):
                    break
            count = len(stats)
            r.sync()
            targets.append(DeviceBuffer(16 * (width + 64) * (height + 64)))
            r.render(targets[-1].ptr.value)
            stats.append(r.prepared_polygon_statistics())
            r.sync()
            results.append(([t.download((height, width, 4), np.float32) for t in targets], stats))
        finally:
            r.close()
            for t in targets:
                t.free()
            monkeypatch.delenv("VKR_PREPARED_POLYGONS_MIB", raising=False)
    (warm_images, warm_stats), (cold_images, cold_stats) = results
    sequence = [s["mode"] for s in warm_stats]
    print(sequence, warm_stats[-1])
    assert sequence[:2] == ["plain", "storing"] and sequence[-1] == "loading"
    assert any(sequence[i] == "loading" and i % 3 != 1 for i in range(2, len(sequence) - 1)), "no launch on another stream loaded while frames were in flight"
    waited = 0
    for index in range(2, len(sequence) - 1):
        # a launch runs plain exactly when it is on another stream than the storing launch (frame 2; the streams take turns)
        # and the query before it found that launch incomplete; on the storing launch's own stream it runs behind it anyway
        found_incomplete = warm_stats[index]["waited"] - warm_stats[index - 1]["waited"]
        assert found_incomplete in (0, 1)
        assert sequence[index] == ("plain" if found_incomplete else "loading"), (index, sequence, warm_stats[index])
        assert not (found_incomplete and index % 3 == 1), (index, sequence)
        waited += found_incomplete
    # once the storing launch has been seen complete, every launch loads
    seen_complete = min(i for i in range(2, len(sequence) - 1) if sequence[i] == "loading" and i % 3 != 1)
    assert all(mode == "loading" for mode in sequence[seen_complete:]), sequence
    assert warm_stats[-1]["launches"] == {"plain": 1 + waited, "storing": 1, "loading": len(sequence) - 2 - waited}
    assert all(s["mode"] == "plain" and s["buffer_bytes"] == 0 for s in cold_stats)
    assert len(warm_images) == len(cold_images)
    for index, (w, c) in enumerate(zip(warm_images, cold_images)):
        assert np.array_equal(w.view(np.uint32), c.view(np.uint32)), (index, sequence)
    assert not np.array_equal(cold_images[0], cold_images[1])


def test_config_3_at_full_size(big_dataset, monkeypatch):
    """BASELINE config 3 at 1920 x 1080 with the noise standing still: frames 3 and 4 (loading) are frame 1 (plain) in every
    bit - the frame that tests/test_gpu_full_size.py compares with the oracle - and the buffer is the 2 040 MiB of DESIGN.md"""
    monkeypatch.delenv("VKR_PREPARED_POLYGONS_MIB", raising=False)
    r = renderer.Renderer()
    try:
        renderer.setup_config(r, 3, big_dataset, acceleration_structure="sah_device")
        r.create_targets()
        r.create_pass()
        r.render_visibility()
        frames = []
        for index in range(4):
            r.render()
            frames.append({"image": r.read_radiance(), "stats": r.prepared_polygon_statistics()})
    finally:
        r.close()
    assert modes(frames) == ["plain", "storing", "loading", "loading"]
    assert frames[-1]["stats"]["buffer_bytes"] == 4 * 16 * 16 * 8160 * 256
    for index in (1, 2, 3):
        a, b = frames[0]["image"].view(np.uint32), frames[index]["image"].view(np.uint32)
        assert np.array_equal(a, b), (index, int((a != b).any(axis=-1).sum()))


def test_a_budget_below_the_buffer(big_dataset, monkeypatch):
    """The four lights of the frame need 4 MiB: with a budget of 3 every launch is plain and nothing is allocated"""
    small, cold = sequences(monkeypatch, lambda: start(big_dataset), [None] * 4, budgets=("3", OFF))
    assert modes(small) == ["plain"] * 4
    for frame in small:
        assert frame["stats"]["buffer_bytes"] == 0 and frame["stats"]["budget_mib"] == 3 and frame["stats"]["launches"]["storing"] == 0
    assert_frames_equal(small, cold)
