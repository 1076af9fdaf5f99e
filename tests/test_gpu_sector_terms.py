"""Sector terms that are kept with the prepared polygons (csrc/kept_polygons.h "Sector terms that are still true",
csrc/prepared_polygons.hip): behind the storing launch a kernel derives, for every
sector that a sample of a decentral polygon can fall into, the eight inverse square roots that depend on the sector alone,
and the launches after it load them instead of computing them.  A loaded term is the term, so every frame must be the
frame of a pass that keeps nothing (VKR_PREPARED_POLYGONS_MIB=0), in every bit: no tolerance anywhere.

The frames, the lights and what they are placed for are those of tests/test_gpu_prepared_polygon_reuse.py (its
docstring), at 64 x 64 pixels - 4 096 threads in 16 blocks.  The set "four" puts into one frame: a central polygon (below
"above"), decentral quads (beside it), a triangle, a quad that the horizon cuts to five vertices - four sectors -
("standing"), whose specular polygon is culled next to it, and a light that adds nothing ("below"); "triangles" is a
pass with V = 4, three sectors per polygon."""
import numpy as np
import pytest

from helpers import DeviceBuffer
from test_gpu_prepared_polygon_reuse import LIGHTS, LIGHT_SETS, moved_vertex, nudged_camera
from vulkan_renderer_amd import renderer, synthetic

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT = 64, 64
THREADS = 4096
STRATEGIES = {"separately": ("diffuse_specular_separately", "balance"), "mis": ("diffuse_specular_mis", "optimal_clamped"),
              "random": ("diffuse_specular_random", "balance")}
# [light][polygon][sector][half][thread]: 2 polygons x (V - 1) sectors x 2 quads of 16 bytes
TERM_BYTES_PER_PAIR = {"four": 2 * 4 * 2 * 16, "triangles": 2 * 3 * 2 * 16}
OFF = "0"
PENTAGON = synthetic.light_spec(synthetic.regular_polygon(5), (-1.8, -0.2, 1.4), (np.pi, 0.0, 0.3), (6, 6, 8), (1.0, 0.8))


def start(dataset, lights="four", strategy="mis", frames_in_flight=1, width=WIDTH, height=HEIGHT, arithmetic=None):
    r = renderer.Renderer(frames_in_flight=frames_in_flight, arithmetic=arithmetic)
    strategies, heuristic = STRATEGIES[strategy]
    renderer.setup_config(r, 3, dataset, width=width, height=height, acceleration_structure="sah_device",
                          sampling_strategies=strategies, mis_heuristic=heuristic, animate_noise=True)
    r.set_lights([PENTAGON] if lights == "pentagon" else [LIGHTS[name] for name in LIGHT_SETS[lights]])
    r.create_targets()
    return r


def set_environment(monkeypatch, budget, terms):
    for name, value in (("VKR_PREPARED_POLYGONS_MIB", budget), ("VKR_SECTOR_TERMS", terms)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def sequences(monkeypatch, begin, steps, runs=((None, None), (OFF, None))):
    """One frame per entry of `steps` (a callable that changes an input before the frame, or None), once per (budget in MiB,
    VKR_SECTOR_TERMS) of `runs` (None: the default) -> per run a list of {"image", "stats", "terms"}.  The noise is
    animated: frame k of every run draws the same numbers."""
    out = []
    for budget, terms in runs:
        set_environment(monkeypatch, budget, terms)
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
                # (read_radiance waits for the frame: a storing launch and its terms have completed when the next frame is planned)
                frames.append({"image": r.read_radiance(), "stats": r.prepared_polygon_statistics(), "terms": r.sector_terms_statistics()})
            out.append(frames)
        finally:
            r.close()
            set_environment(monkeypatch, None, None)
    return out


def modes(frames):
    return [f["stats"]["mode"] for f in frames]


def loads(frames):
    """(with terms, without) of each frame's launch"""
    counts = [(0, 0)] + [(f["terms"]["loaded_with_terms"], f["terms"]["loaded_without_terms"]) for f in frames]
    return [(b[0] - a[0], b[1] - a[1]) for a, b in zip(counts, counts[1:])]


def assert_frames_equal(warm, cold):
    assert len(warm) == len(cold)
    for index, (w, c) in enumerate(zip(warm, cold)):
        a, b = w["image"].view(np.uint32), c["image"].view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (index, w["stats"]["mode"], w["terms"], int((a != b).any(axis=-1).sum()))
    # animated noise: the frames of a sequence differ from each other, or equal frames would say nothing
    assert not np.array_equal(cold[0]["image"], cold[1]["image"])
    for frame in cold:
        assert frame["stats"]["mode"] == "plain" and frame["stats"]["buffer_bytes"] == 0 and frame["terms"] == {"buffer_bytes": 0, "loaded_with_terms": 0, "loaded_without_terms": 0}


@pytest.mark.parametrize("lights", ["four", "triangles"])
@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
def test_five_frames_standing_still(big_dataset, monkeypatch, strategy, lights):
    """plain, storing (and the terms kernel), then three launches that load with terms - and every frame is the frame of a
    pass that keeps nothing"""
    warm, cold = sequences(monkeypatch, lambda: start(big_dataset, lights, strategy), [None] * 5)
    assert modes(warm) == ["plain", "storing", "loading", "loading", "loading"]
    assert loads(warm) == [(0, 0), (0, 0), (1, 0), (1, 0), (1, 0)]
    assert warm[0]["terms"]["buffer_bytes"] == 0
    for frame in warm[1:]:
        assert frame["terms"]["buffer_bytes"] == len(LIGHT_SETS[lights]) * TERM_BYTES_PER_PAIR[lights] * THREADS
    assert_frames_equal(warm, cold)
    image = cold[0]["image"]
    assert 0.02 < (image[..., :3] == 0.0).all(axis=-1).mean() < 0.98, "the frame should hold lit pixels and sky or unlit ones"


@pytest.mark.parametrize("lights", ["four", "triangles"])
def test_polynomial_arithmetic(big_dataset, monkeypatch, lights):
    """the "exact" mode fills and loads its terms with kernels of its own: its inverse square root is another one"""
    warm, cold = sequences(monkeypatch, lambda: start(big_dataset, lights, arithmetic="exact"), [None] * 4)
    assert modes(warm) == ["plain", "storing", "loading", "loading"]
    assert loads(warm) == [(0, 0), (0, 0), (1, 0), (1, 0)]
    assert_frames_equal(warm, cold)


@pytest.mark.parametrize("what", ["fast", "pentagon"])
def test_no_terms_where_no_polygons_are_kept(big_dataset, monkeypatch, what):
    """the fast mode and polygons of six vertices or more (V >= 6: a pentagon and its clipped vertex) have no storing and no
    loading kernels, and so no terms"""
    begin = (lambda: start(big_dataset, arithmetic="fast")) if what == "fast" else (lambda: start(big_dataset, "pentagon"))
    warm, cold = sequences(monkeypatch, begin, [None] * 3)
    assert modes(warm) == ["plain"] * 3
    for frame in warm:
        assert frame["terms"] == {"buffer_bytes": 0, "loaded_with_terms": 0, "loaded_without_terms": 0}
    assert_frames_equal(warm, cold)


@pytest.mark.parametrize("runs", [("6", None), (None, "0")], ids=["budget", "switched_off"])
def test_loading_without_terms(big_dataset, monkeypatch, runs):
    """The polygons of the frame take 4 MiB and their terms 4 more: a budget of 6 MiB holds the polygons alone, and
    VKR_SECTOR_TERMS=0 keeps no terms whatever the budget.  The launches load as they did before there were terms."""
    warm, cold = sequences(monkeypatch, lambda: start(big_dataset), [None] * 4, runs=(runs, (OFF, None)))
    assert modes(warm) == ["plain", "storing", "loading", "loading"]
    assert loads(warm) == [(0, 0), (0, 0), (0, 1), (0, 1)]
    for frame in warm:
        assert frame["terms"]["buffer_bytes"] == 0
    assert warm[-1]["stats"]["buffer_bytes"] == 4 * 16 * 16 * THREADS
    assert_frames_equal(warm, cold)


def test_the_terms_are_forgotten_with_the_polygons(big_dataset, monkeypatch):
    """A light vertex moves, later the camera: the launch after either is plain, the next one stores polygons and terms anew,
    and the standing frames behind it load with terms - all of them the frames of a pass that keeps nothing."""
    warm, cold = sequences(monkeypatch, lambda: start(big_dataset), [None] * 3 + [moved_vertex] + [None] * 2 + [nudged_camera] + [None] * 3)
    assert modes(warm) == ["plain", "storing", "loading"] * 3 + ["loading"]
    assert loads(warm) == [(0, 0), (0, 0), (1, 0)] * 3 + [(1, 0)]
    assert_frames_equal(warm, cold)


def test_three_frames_in_flight(big_dataset, monkeypatch):
    """Frames of 640 x 368 are submitted without a wait in between, each into a target of its own, until one of them has
    loaded on another stream than the storing launch's while others were in flight, and two more have followed it.  The event
    that lets other streams load is recorded behind the terms kernel: a launch on another stream that finds it incomplete
    runs plain (and is counted as having waited), and none loads - with terms or without - before it has been seen
    complete.  No launch ever loads without terms, and EVERY frame is the frame of a pass that keeps nothing: a launch that
    loads terms before they are written samples with whatever the buffer holds."""
    width, height = 640, 368
    results = []
    count = None
    for budget in (None, OFF):
        set_environment(monkeypatch, budget, None)
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
                stats.append(dict(r.prepared_polygon_statistics(), terms=r.sector_terms_statistics()))
                # (the storing launch is frame 1; the streams take turns)
                if first_loading is None and stats[-1]["mode"] == "loading" and (len(stats) - 1) % 3 != 1:
                    first_loading = len(stats) - 1
                if count is None and first_loading is not None and len(stats) >= max(first_loading + 3, 6):
                    break
            count = len(stats)
            r.sync()
            results.append(([t.download((height, width, 4), np.float32) for t in targets], stats))
        finally:
            r.close()
            for t in targets:
                t.free()
            set_environment(monkeypatch, None, None)
    (warm_images, warm_stats), (cold_images, cold_stats) = results
    sequence = [s["mode"] for s in warm_stats]
    print(sequence, warm_stats[-1])
    assert sequence[:2] == ["plain", "storing"]
    assert any(sequence[i] == "loading" and i % 3 != 1 for i in range(2, len(sequence))), "no launch on another stream loaded while frames were in flight"
    with_terms = 0
    for index in range(2, len(sequence)):
        found_incomplete = warm_stats[index]["waited"] - warm_stats[index - 1]["waited"]
        loaded_with = warm_stats[index]["terms"]["loaded_with_terms"] - warm_stats[index - 1]["terms"]["loaded_with_terms"]
        assert found_incomplete in (0, 1)
        # on another stream than the storing launch's: plain until the event behind the terms kernel has been seen complete
        assert sequence[index] == ("plain" if found_incomplete else "loading"), (index, sequence, warm_stats[index])
        assert not (found_incomplete and index % 3 == 1), (index, sequence)
        assert loaded_with == (0 if found_incomplete else 1), (index, sequence, warm_stats[index])
        assert warm_stats[index]["terms"]["loaded_without_terms"] == 0
        with_terms += loaded_with
    assert warm_stats[-1]["launches"]["loading"] == with_terms
    # at V = 5 a pair's terms take what its polygons take: 256 bytes
    assert TERM_BYTES_PER_PAIR["four"] == 16 * 16 and warm_stats[-1]["terms"]["buffer_bytes"] == warm_stats[-1]["buffer_bytes"] != 0
    assert all(s["mode"] == "plain" and s["terms"]["buffer_bytes"] == 0 for s in cold_stats)
    assert len(warm_images) == len(cold_images)
    for index, (w, c) in enumerate(zip(warm_images, cold_images)):
        assert np.array_equal(w.view(np.uint32), c.view(np.uint32)), (index, sequence)
    assert not np.array_equal(cold_images[0], cold_images[1])
