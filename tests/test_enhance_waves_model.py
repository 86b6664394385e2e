"""CPU: the index arithmetic of a packed batch (spec64.waves_*).  The kernel-way model -- the searches, rs(u) and the
clamps of k_lps_analysis_seg, k_lps_stream_seg, k_ola_seg and the engine's chunk loop -- equals the model built per
utterance, on every batch the GPU tests run and on a seeded sweep; every planted slip changes a mapped index in each
GPU configuration that claims to discriminate it, so a kernel with that slip could not pass that test; and each GPU
test's docstring names the slips its batches discriminate.  No device is touched."""
import importlib

import numpy as np
import pytest

import spec64

CONFIGS = spec64.waves_gpu_configs()


def variants(cfg):
    for cap in cfg["caps"]:
        for lookup in cfg["lookups"]:
            for base in cfg["bases"]:
                yield cap, lookup, base


def test_the_stream_model_is_the_context_window_of_every_frame():
    """what the model itself must mean: rows first[i] .. first[i] + ctx - 1 of a chunk's stream are the frames
    clamp(t - half .. t + half) of the utterance that owns packed frame a + i = frame_off[u] + t"""
    frames = [1, 2, 3, 5, 17, 30, 1, 1, 4]
    _, fo, _ = spec64.waves_layout64(frames, 8)
    for ctx in (1, 3, 7, 11):
        for cap in (1, 2, 5, 7, 33, 64, 1000):
            chunks = spec64.waves_chunks(fo, cap)
            for (a, n), (src, first) in zip(chunks, spec64.waves_stream_model(fo, ctx, cap)):
                for i in range(n):
                    u = max(v for v in range(len(frames)) if fo[v] <= a + i)
                    want = fo[u] + spec64.context_index(frames[u], ctx)[a + i - fo[u]]
                    assert src[first[i]:first[i] + ctx].tolist() == want.tolist(), (ctx, cap, a, i)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_kernel_way_equals_per_utterance_on_the_gpu_configurations(name):
    cfg = CONFIGS[name]
    for cap, lookup, base in variants(cfg):
        want = spec64.waves_index_model(cfg["frames"], cfg["fs"], cfg["ctx"], cap, base)
        got = spec64.waves_index_kernel(cfg["frames"], cfg["fs"], cfg["ctx"], cap, base, lookup)
        assert spec64.waves_same_index(got, want), (name, cap, lookup, base)


def test_kernel_way_equals_per_utterance_on_a_seeded_sweep():
    """utterances of 1 to 40 frames, 1 to 5000 of them (the count drawn on a log scale, the longest length lowered
    so a batch stays below 20000 frames), every context, capacities from 1 to beyond the total, both lookups, a base"""
    rng = np.random.default_rng(20260)
    counts = [1, 2, 3, 5000] + [int(round(np.exp(x))) for x in rng.uniform(0, np.log(5000), 20)]
    seen = 0
    for k, n_utts in enumerate(counts):
        longest = int(max(1, min(40, 20000 // n_utts)))
        frames = rng.integers(1, longest + 1, n_utts).tolist()
        total, ctx = sum(frames), (1, 3, 7, 11)[k % 4]
        fs = (8, 11, 16)[k % 3] if total < 4000 else 8
        caps = {total + 5, total, max(1, total - 1), int(rng.integers(1, total + 1)), 257}
        if total <= 3000:
            caps.add(1)
        for cap in sorted(caps):
            base = int(rng.integers(0, 3)) * 501
            want = spec64.waves_index_model(frames, fs, ctx, cap, base)
            for lookup in ("search", "table"):
                got = spec64.waves_index_kernel(frames, fs, ctx, cap, base, lookup)
                assert spec64.waves_same_index(got, want), (n_utts, ctx, cap, lookup)
                seen += 1
    assert seen >= 200


@pytest.mark.parametrize("ctx", [1, 3, 7, 11])
def test_kernel_way_equals_per_utterance_for_every_context(ctx):
    rng = np.random.default_rng(ctx)
    for n_utts in (1, 2, 7, 64, 65, 500):
        frames = rng.integers(1, 41, n_utts).tolist()
        for cap in (1, 2, 40, 41, 333, sum(frames), sum(frames) + 1):
            if cap == 1 and n_utts > 65:
                continue
            want = spec64.waves_index_model(frames, 11, ctx, cap)
            for lookup in ("search", "table"):
                assert spec64.waves_same_index(spec64.waves_index_kernel(frames, 11, ctx, cap, 0, lookup), want)


def discriminating(cfg, slip):
    """the (cap, lookup, base) variants of a configuration in which the slip changes a mapped index"""
    seen = []
    for cap, lookup, base in variants(cfg):
        want = spec64.waves_index_model(cfg["frames"], cfg["fs"], cfg["ctx"], cap, base)
        got = spec64.waves_index_kernel(cfg["frames"], cfg["fs"], cfg["ctx"], cap, base, lookup, slip)
        if not spec64.waves_same_index(got, want):
            seen.append((cap, lookup, base))
    return seen


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_every_claimed_slip_changes_a_mapped_index(name):
    cfg = CONFIGS[name]
    assert cfg["slips"] and set(cfg["slips"]) <= set(spec64.WAVES_SLIPS)
    for slip in cfg["slips"]:
        seen = discriminating(cfg, slip)
        print("slip %-22s caught by %-15s in %d of %d variants, e.g. cap %d lookup %s base %d"
              % (slip, name, len(seen), len(list(variants(cfg))), *(seen[0] if seen else (-1, "-", -1))))
        assert seen, (name, slip)
        if slip == "table_plus_1":                                     # only the table engines can see it
            assert all(lookup == "table" for _, lookup, _ in seen)
        if slip == "wave_off_not_rebased":
            assert len(seen) == len(list(variants(cfg))) and all(base != 0 for _, _, base in seen)


def test_every_slip_is_claimed_by_a_gpu_configuration_and_named_in_its_docstring():
    gpu_tests = importlib.import_module("test_gpu_enhance_waves")
    claimed = {}
    for name, cfg in CONFIGS.items():
        doc = getattr(gpu_tests, cfg["test"]).__doc__
        for slip in cfg["slips"]:
            assert slip in doc, (cfg["test"], slip)
            claimed.setdefault(slip, []).append(name)
    for slip in spec64.WAVES_SLIPS:
        print("slip %-22s claimed by %s" % (slip, ", ".join(claimed.get(slip, []))))
    assert sorted(claimed) == sorted(spec64.WAVES_SLIPS)


def test_a_slip_that_hangs_a_search_is_reported_not_looped():
    _, fo, _ = spec64.waves_layout64([3, 4], 8)
    got = spec64.waves_analysis_kernel(np.array([0, 640, 1408]), fo, 8, slip="search_bias")
    assert (got == -1).any()


def test_the_many_utterance_batches_reach_the_depth_and_rows_growth_regime():
    """n_utts >= 2048 (searches 11 and 12 levels deep, one count odd, one a power of two), and with capacities 257 and
    1000 a full chunk that touches hundreds of utterances; with 257 its stream is at least five times its frames"""
    for name, odd in (("many_odd", 1), ("many_even", 0)):
        cfg = CONFIGS[name]
        assert len(cfg["frames"]) >= 2048 and len(cfg["frames"]) % 2 == odd
        _, fo, _ = spec64.waves_layout64(cfg["frames"], cfg["fs"])
        assert any(n == 257 and rows >= 5 * n and touched >= 100
                   for n, rows, touched in spec64.waves_rows_per_chunk(fo, cfg["ctx"], 257))
        assert any(n == 1000 and touched >= 300 for n, _, touched in spec64.waves_rows_per_chunk(fo, cfg["ctx"], 1000))
        assert sum(f >= 200 for f in cfg["frames"]) >= 5 and max(f for f in cfg["frames"] if f < 200) == 4
