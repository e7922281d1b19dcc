"""render()'s per-stream sort state driven the way training drives it: scripted SEQUENCES of different views on one
stream, where the route of every frame is chosen from what the earlier frames left behind (pair-count estimate, held
capacity, wide-depth counter, the keyed sort workspace and its control words, pinned count words, the pre-cleared
backward accumulator).

Every frame is held to the bars of test_projection_keys_the_sort - pair count, tile ranges and index list equal to the
oracle's, the image bit-equal - and to the host model of tests/sortstate_ref.py: the C entry points rasterizer calls
(recorded by wrapping `rasterizer.lib`), the capacity it passes, the number of blocking re-sorts and blends, and the
state it leaves must be what the model predicts from the oracle's counts alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sortstate_ref as M
from util import load_parity, max_rel_err, np_, oracle_backward, oracle_forward

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4     # the bar of test_gpu_parity.py: every gradient within 1e-4 of its tensor's scale
DEG = 1
WIDE_SCALE = 5000.0

_WATCHED = {M.PROJECT, M.PROJECT_KEYED, M.COUNT, M.COUNT_WIDE, M.PAIRS, M.KEYED, M.KEYED_ORDERED, M.WIDE, M.TILE_ORDER,
            "cugs_sort_pairs_predicted", "cugs_project_forward_geometry"}
_PREDICTED = {M.KEYED, M.KEYED_ORDERED, M.WIDE, "cugs_sort_pairs_predicted"}
_BLEND = "cugs_rasterize_forward_opts"


# --------------------------------------------------------------------------------------
# scenes: built and sent through the oracle once, shared, never modified
# --------------------------------------------------------------------------------------
def _gaussians(pkg, n, w, h, seed, mu_s):
    return pkg.scene.make_gaussians(n, w, h, sh_degree=DEG, seed=seed, mu_s=mu_s)


def _arrays(pkg, name):
    S = lambda: _gaussians(pkg, 20000, 640, 360, 101, -4.6)
    if name in ("S", "R"):
        return S()
    if name == "D":
        return _gaussians(pkg, 20000, 640, 360, 101, -3.0)
    if name == "W":                               # everything 5000 times farther and larger: the same image
        a = S()
        a["positions"] = (a["positions"] * np.float32(WIDE_SCALE)).astype(np.float32)
        a["scales"] = (a["scales"] + np.float32(np.log(WIDE_SCALE))).astype(np.float32)
        return a
    if name == "G":                               # grown: 6000 more from another seed
        a, b = S(), _gaussians(pkg, 6000, 640, 360, 202, -4.6)
        return {k: np.concatenate([a[k], b[k]], axis=0) for k in a}
    if name == "K":                               # shrunk
        return {k: v[:12000].copy() for k, v in S().items()}
    if name == "R6":
        return {k: v[:6000].copy() for k, v in S().items()}
    if name == "L":
        return _gaussians(pkg, 3000, 2064, 32, 303, -2.0)
    if name == "XL":
        return _gaussians(pkg, 3000, 4112, 16, 404, -2.0)
    if name == "Z":                               # every splat behind the camera: no pairs
        a = S()
        a["positions"][:, 2] = -np.abs(a["positions"][:, 2])
        return a
    raise KeyError(name)


_SIZE = {"S": (640, 360), "D": (640, 360), "W": (640, 360), "G": (640, 360), "K": (640, 360), "Z": (640, 360),
         "R": (320, 200), "R6": (320, 200), "L": (2064, 32), "XL": (4112, 16)}


@functools.lru_cache(maxsize=None)
def scene(name):
    import __graft_entry__ as ge
    pkg, orc = ge.load_package(), ge.load_oracle()
    w, h = _SIZE[name]
    arrays = _arrays(pkg, name)
    cam = pkg.scene.make_camera(w, h)
    ref = oracle_forward(orc, arrays, cam, degree=DEG)
    for v in (*arrays.values(), *(a for a in ref.values() if isinstance(a, np.ndarray))):
        v.setflags(write=False)
    n = int(arrays["positions"].shape[0])
    return dict(name=name, arrays=arrays, cam=cam, ref=ref, n=n, w=w, h=h, pairs=int(ref["total_pairs"]),
                wide=M.out_of_narrow_range(ref["depths"], ref["tiles_touched"], ref["radii"]))


def _cap(pairs):
    """The capacity of a fresh prediction of `pairs`."""
    return int(pairs * M.MARGIN[0]) + M.MARGIN[1]


def test_scenes_reach_the_routes_they_are_meant_for(pkg, orc):
    """What the sequences below rely on, asserted from the oracle's counts (printed: pairs and fresh capacity)."""
    s = {k: scene(k) for k in _SIZE}
    for k, v in s.items():
        print(f"scene {k:2s}: N {v['n']:6d}  {v['w']}x{v['h']}  pairs {v['pairs']:8d}  pairs/N {v['pairs'] / v['n']:6.2f}  "
              f"capacity {_cap(v['pairs']):8d}  out of narrow range: {v['wide']}")
    S, D, W, G, K, L, XL, Z, R, R6 = (s[k] for k in ("S", "D", "W", "G", "K", "L", "XL", "Z", "R", "R6"))
    n = S["n"]
    assert S["pairs"] < 13 * n and _cap(S["pairs"]) < 13 * n                     # the unstaged direct scatter
    assert M.pair_route(n, 640, 360, _cap(S["pairs"]), True) == "direct"
    assert D["pairs"] >= 13 * n and D["pairs"] > _cap(S["pairs"])                # staged, and S -> D is a miss
    assert M.pair_route(n, 640, 360, _cap(D["pairs"]), True) == "direct_staged"
    assert S["pairs"] <= _cap(D["pairs"]) and not S["wide"] and not D["wide"]
    # W is S's image from depths beyond 13 107
    assert W["wide"] and W["ref"]["depths"][W["ref"]["tiles_touched"] > 0].max() > 13107.0
    assert np.array_equal(W["ref"]["tiles_touched"], S["ref"]["tiles_touched"])
    assert W["pairs"] == S["pairs"] and np.array_equal(W["ref"]["tile_ranges"], S["ref"]["tile_ranges"])
    assert G["n"] == n + 6000 and K["n"] == 12000 and K["pairs"] < S["pairs"] < G["pairs"]
    # 129 / 257 tile columns: no packed rectangles, no direct route; L the column path (at 3000 Gaussians the 64 Ki
    # margin alone is 13 per Gaussian, so on whatever capacity it inherits), XL never
    assert M.pair_route(L["n"], L["w"], L["h"], _cap(L["pairs"]), True) == "column" and L["pairs"] >= 13 * L["n"]
    assert M.pair_route(XL["n"], XL["w"], XL["h"], _cap(XL["pairs"]), True) == "radix" and XL["pairs"] > 0
    assert Z["pairs"] == 0 and not Z["wide"]
    assert 0 < R6["pairs"] < R["pairs"] and not R["wide"] and not R6["wide"]


# --------------------------------------------------------------------------------------
# the recorder and the frame runner
# --------------------------------------------------------------------------------------
class _Spy:
    """Stands in for rasterizer.lib: every call goes through; the watched ones are recorded with the stream they were
    made on and, for the predicted sorts, the capacity passed."""

    def __init__(self, lib, dev):
        self._lib, self._dev, self.calls = lib, dev, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _WATCHED and name != _BLEND:
            return fn

        def wrapped(*args):
            stream = int(torch.cuda.current_stream(self._dev).cuda_stream)
            self.calls.append((name, int(args[1]) if name in _PREDICTED else None, stream))
            return fn(*args)
        return wrapped

    def take(self, stream):
        mine = [c for c in self.calls if c[2] == stream]
        self.calls = [c for c in self.calls if c[2] != stream]
        return mine


def _assert_frame_is_the_oracles(out, sc, label):
    ref = sc["ref"]
    assert out.total_pairs == ref["total_pairs"], label
    assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"]), label
    assert np.array_equal(np_(out.gaussian_indices), ref["values"]), label
    assert np.array_equal(np_(out.n_contrib), ref["n_contrib"]), label
    assert np.array_equal(np_(out.color).view(np.uint32), ref["color"].view(np.uint32)), label


class _Stream:
    """One stream's script: renders frames, checks each against the oracle and against the model."""

    def __init__(self, pkg, dev, spy):
        self.pkg, self.dev, self.spy, self.R = pkg, dev, spy, pkg.rasterizer
        self.key = self.R._skey(torch.device(dev))
        self.model = M.StreamModel()
        self.models, self.trace, self.index = {}, [], 0
        self.settings = pkg.RenderSettings(active_sh_degree=DEG)
        # the stream starts as a new training run finds it: no prediction, no held capacity, no sort workspaces (the
        # suite's earlier tests leave gigabytes there, which no sequence would ever outgrow); put back afterwards
        self._saved = {d: getattr(self.R, d).pop(self.key, None) for d in ("_last_pairs", "_held_capacity")}
        self._saved_ws = {k: self.R._workspaces.pop((self.key, k), None) for k in ("n", "p")}

    def restore(self):
        for d, v in self._saved.items():
            getattr(self.R, d).pop(self.key, None)
            if v is not None:
                getattr(self.R, d)[self.key] = v
        for k, v in self._saved_ws.items():
            self.R._workspaces.pop((self.key, k), None)
            if v is not None:
                self.R._workspaces[(self.key, k)] = v

    def gpu_model(self, name):
        if name not in self.models:
            self.models[name] = self.pkg.scene.to_model(scene(name)["arrays"], self.dev)
        return self.models[name]

    def _check_calls(self, exp, label, blends):
        calls = self.spy.take(self.key[1])
        names = tuple(c[0] for c in calls if c[0] != _BLEND)
        line = f"{label}: {' '.join(n.replace('cugs_', '') for n in names)}  capacity {exp.capacity}  " \
               f"valid {exp.valid}  state {self.R._last_pairs.get(self.key)}/{self.R._held_capacity.get(self.key)}/" \
               f"{self.R._wide_depth.get(self.key, 0)}"
        self.trace.append(line)
        print(line)
        assert names == exp.calls, (label, names, exp.calls)
        caps = [c[1] for c in calls if c[0] in _PREDICTED]
        assert caps == ([] if exp.capacity is None else [exp.capacity]), (label, caps, exp.capacity)
        predicted_at = [i for i, n in enumerate(names) if n in _PREDICTED]
        resorts = sum(1 for n in names[predicted_at[0]:] if n in (M.COUNT, M.COUNT_WIDE)) if predicted_at else 0
        assert resorts == exp.resorts, (label, resorts, exp.resorts)
        assert sum(1 for c in calls if c[0] == _BLEND) == blends, label
        R, m = self.R, self.model
        assert (R._last_pairs.get(self.key), R._held_capacity.get(self.key), R._wide_depth.get(self.key, 0)) == \
            (m.estimate, m.held, m.wide), label

    def frame(self, name, mode="block"):
        """mode: "block", "defer" (defer_count=True; a predicted miss must raise from wait() and is retried at once,
        as a training loop does), "eval" (for_backward=False).  Returns the finished RenderOutput."""
        sc = scene(name)
        self.index += 1
        label = f"frame {self.index} {name} {mode}"
        exp = self.model.frame(sc["pairs"], sc["wide"], sc["n"], sc["w"], sc["h"])
        gm = self.gpu_model(name)
        if mode != "defer":
            out = self.pkg.render(gm, sc["cam"], self.settings, for_backward=mode != "eval")
            self._check_calls(exp, label, blends=1 + exp.resorts)          # a miss costs a second blend
            assert (out.zeroed_accum is None) == (mode == "eval"), label
        else:
            out = self.pkg.render(gm, sc["cam"], self.settings, defer_count=True)
            assert (out.pending is not None) == (exp.capacity is not None), label
            if exp.valid:
                out.wait()
                self._check_calls(exp, label, blends=1)
            else:
                with pytest.raises(self.pkg.PredictionMiss, match="general" if exp.wide_found else "too small"):
                    out.wait()
                self._check_calls(exp, label, blends=1)
                retry = self.frame(name, "defer")
                assert self.model.history[-1].valid, label
                return retry
        _assert_frame_is_the_oracles(out, sc, label)
        return out

    def range_flag(self):
        """The range flag of this stream's keyed sort workspace (SortCtl::range_flag, byte 24 of the control block)."""
        ws = self.R._workspaces[(self.key, "n")]
        return int(ws[24:28].view(torch.int32).item())


@pytest.fixture
def stream(pkg, dev, monkeypatch):
    R = pkg.rasterizer
    spy = _Spy(R.lib, dev)
    monkeypatch.setattr(R, "lib", spy)
    st = _Stream(pkg, dev, spy)
    try:
        yield st
    finally:
        st.restore()


@functools.lru_cache(maxsize=None)
def _oracle_grads(name):
    import __graft_entry__ as ge
    sc = scene(name)
    g = ge.load_package().scene.make_dl_dcolor(sc["w"], sc["h"])
    refb = oracle_backward(ge.load_oracle(), g, sc["ref"], sc["arrays"], sc["cam"])
    return g, refb


def _assert_gradients_are_the_oracles(st, out, name, label):
    sc = scene(name)
    g, refb = _oracle_grads(name)
    grads = st.pkg.render_backward(torch.from_numpy(g).to(st.dev), out, st.gpu_model(name), sc["cam"], st.settings)
    names = ("dL_dpositions", "dL_drotations", "dL_dscales", "dL_dopacities", "dL_dsh_coeffs", "dL_dmeans_2d")
    par = load_parity()
    rep = par.gradient_report({k: np_(getattr(grads, k)) for k in names}, refb, names)
    print(par.format_report(rep, f"{label}: render_backward vs oracle"))
    for k, v in rep["per_tensor"].items():
        assert v["over_scale"] <= GRAD_TOL, (label, k, v)
        got = np_(getattr(grads, k)).reshape(refb[k].shape)
        assert max_rel_err(got, refb[k], floor_frac=1e-3) <= 20 * GRAD_TOL, (label, k)


# --------------------------------------------------------------------------------------
# the sequences
# --------------------------------------------------------------------------------------
def test_dense_and_sparse_views_miss_and_recover(stream):
    """S S D D S S S: the dense view overflows the sparse views' capacity (one re-sort, a second blend over the
    accumulator the first one cleared), the next dense frame fits, and the sparse frames after it run on the dense
    view's held capacity - the staged scatter on few pairs.  Blocking and deferred frames alternate."""
    st = stream
    st.frame("S", "block")
    st.frame("S", "defer")
    out = st.frame("D", "block")
    assert not st.model.history[-1].valid and st.model.history[-1].route == "direct"
    _assert_gradients_are_the_oracles(st, out, "D", "the missed frame, blended twice")
    out = st.frame("D", "defer")
    assert st.model.history[-1].valid and st.model.history[-1].route == "direct_staged"
    _assert_gradients_are_the_oracles(st, out, "D", "first frame after the miss")
    out = st.frame("S", "block")
    assert st.model.history[-1].route == "direct_staged"              # the stale, held capacity
    _assert_gradients_are_the_oracles(st, out, "S", "first sparse frame after the dense ones")
    st.frame("S", "defer")
    st.frame("S", "eval")
    assert all(f.valid for f in st.model.history[3:])


def test_held_capacity_is_released_and_a_deferred_miss_recovers(stream):
    """Dense -> sparse: the capacity is held while the estimate decays 3 % a frame and released once it has fallen below
    80 %; sparse frames run the staged scatter until then and the unstaged one afterwards.  Then the dense view again,
    deferred: wait() raises PredictionMiss, the retry is the oracle's frame."""
    st = stream
    st.frame("D", "block")
    st.frame("D", "defer")
    held = st.model.held
    frames = 0
    while st.model.history[-1].route != "direct":
        st.frame("S", ("defer", "block", "eval")[frames % 3])
        frames += 1
        assert frames <= 100
    caps = [f.capacity for f in st.model.history[2:]]
    assert caps[0] == held and caps[-1] < held and sorted(caps, reverse=True) == caps
    print(f"capacity {held} released after {caps.count(held)} sparse frames; unstaged again after {frames}")
    st.frame("S", "defer")
    before = len(st.model.history)
    out = st.frame("D", "defer")                                       # miss, PredictionMiss, retry
    assert [f.valid for f in st.model.history[before:]] == [False, True]
    _assert_gradients_are_the_oracles(st, out, "D", "the retry of a deferred miss")


def test_tile_order_threshold_follows_the_estimate(stream, monkeypatch):
    """The keyed sort writes the blend's tile order itself once the estimate reaches the threshold; the general route
    and the re-sort of a miss add the one-launch order."""
    st = stream
    monkeypatch.setattr(st.R, "TILE_ORDER_MIN_PAIRS", scene("D")["pairs"])
    monkeypatch.setattr(M, "TILE_ORDER_MIN_PAIRS", scene("D")["pairs"])
    st.frame("S")
    st.frame("D")                                                      # miss; the estimate reaches the threshold
    out = st.frame("D")
    assert st.model.history[-1].calls == (M.PROJECT_KEYED, M.KEYED_ORDERED) and out.tile_order is not None
    st.R._wide_depth[st.key] = st.model.wide = 1                      # the last sort of a hold
    out = st.frame("D", "defer")
    assert st.model.history[-1].calls == (M.PROJECT, M.WIDE, M.TILE_ORDER) and out.tile_order is not None
    out = st.frame("S")                                                # the estimate is still the dense view's
    assert st.model.history[-1].calls == (M.PROJECT_KEYED, M.KEYED_ORDERED) and out.tile_order is not None
    out = st.frame("G", "defer")                                       # ... and 3 % lower now: below the threshold
    assert st.model.history[-1].calls == (M.PROJECT_KEYED, M.KEYED) and out.tile_order is None


def test_wide_depth_hold_runs_out_and_the_probe_succeeds(stream):
    """S W W W S S, then in-range frames until the hold has run out by itself, then the probe of the narrow route with
    an in-range view: it must be valid - no re-sort, the counter stays 0 - and the sorts after it stay narrow.  While
    the stream is on the general route the projection must not key the sort: the range flag a keyed projection of an
    out-of-range view sets is only consumed by a narrow sort."""
    st = stream
    st.frame("S", "block")
    st.frame("W", "defer")                                             # narrow -> wide: -1, PredictionMiss, retry on the general route
    assert [f.valid for f in st.model.history[1:]] == [False, True] and st.model.history[1].wide_found
    assert st.model.wide == M.WIDE_DEPTH_HOLD - 1
    st.frame("W", "block")                                             # wide without a miss
    assert st.range_flag() == 0
    st.frame("S", "defer")                                             # in range, inside the hold: the general route
    st.frame("S", "eval")
    assert all(f.valid and f.calls == (M.PROJECT, M.WIDE) for f in st.model.history[2:])
    assert st.range_flag() == 0
    while st.model.wide > 0:                                           # the hold runs out for real
        st.frame("R6", "block" if st.model.wide % 2 else "defer")
    assert len(st.model.history) == 2 + M.WIDE_DEPTH_HOLD
    probe = len(st.model.history)
    st.frame("S", "defer")                                             # the probe
    f = st.model.history[probe]
    assert f.calls == (M.PROJECT_KEYED, M.KEYED) and f.valid and f.resorts == 0
    assert st.R._wide_depth.get(st.key, 0) == 0 and len(st.model.history) == probe + 1
    st.frame("S", "block")
    # a plain unkeyed sort on the same stream: no spurious repeat on the general route (the flag is clear), the
    # oracle's order, and through the predicted entry a valid count
    assert st.range_flag() == 0
    ref = scene("S")["ref"]
    t = lambda k: torch.from_numpy(ref[k]).to(st.dev)
    args = (t("means_2d"), t("depths"), t("radii"), t("tiles_touched"), 640, 360)
    st.spy.take(st.key[1])
    srt = st.pkg.sort_gaussians(*args)
    pend = st.R.sort_gaussians_predicted(*args, want_keys=True)
    srt2, valid = pend.finish()
    names = tuple(c[0] for c in st.spy.take(st.key[1]))
    assert names == (M.COUNT, M.PAIRS, "cugs_sort_pairs_predicted"), names
    assert valid and st.R._wide_depth.get(st.key, 0) == 0
    for out in (srt, srt2):
        assert out.total_pairs == ref["total_pairs"]
        assert np.array_equal(np_(out.gaussian_keys_sorted).view(np.uint64), ref["keys"])
        assert np.array_equal(np_(out.gaussian_values_sorted), ref["values"])
        assert np.array_equal(np_(out.tile_ranges), ref["tile_ranges"])
    # and a view that is wide when the narrow route is probed starts the hold over
    st.model.estimate = st.R._last_pairs[st.key]                       # (the unkeyed predicted sort above moved it)
    st.frame("W", "block")
    assert st.model.wide == M.WIDE_DEPTH_HOLD and not st.model.history[-1].valid


def test_geometry_changes_on_one_stream(stream, dev):
    """S R S L XL S K G S Z S, the empty model, S: image size and Gaussian count change under a live prediction - the
    N-level workspace is re-carved, its control words and the pinned count slots carry over."""
    st = stream
    modes = ("block", "defer", "eval")
    for i, name in enumerate(("S", "R", "S", "L", "XL", "S", "K", "G", "S", "Z", "S")):
        if name == "G":
            # G no longer fits the stream's N-level workspace: the host allocates a new one, whose control words (the
            # range flag among them) must start out zero whatever the block held before.  A block of the size the host
            # will ask for, filled with ones and freed, is what the caching allocator hands out next.
            old = st.R._workspaces[(st.key, "n")]
            need = int(st.R.lib.cugs_sort_workspace_bytes(scene("G")["n"]))
            assert old.numel() < need
            poison = torch.full((int(need * 1.25) + 4096,), 255, dtype=torch.uint8, device=dev)
            del poison
        st.frame(name, modes[i % 3])
        if name == "G":
            assert st.R._workspaces[(st.key, "n")].data_ptr() != old.data_ptr() and st.model.history[-1].valid
            del old
    # the empty model: not sorted at all, the image is the background, the state stays
    f32 = dict(dtype=torch.float32, device=dev)
    empty = st.pkg.GaussianModel(torch.zeros((0, 3), **f32), torch.zeros((0, 3, 4), **f32), torch.zeros((0, 1), **f32),
                                 torch.zeros((0, 4), **f32), torch.zeros((0, 3), **f32))
    exp = st.model.frame(0, False, 0, 640, 360)
    settings = st.pkg.RenderSettings(background=[0.25, 0.5, 0.75], active_sh_degree=DEG)
    out = st.pkg.render(empty, scene("S")["cam"], settings, defer_count=True)
    st._check_calls(exp, "empty model", blends=0)
    assert out.pending is None and out.total_pairs == 0 and tuple(out.color.shape) == (360, 640, 3)
    assert bool((out.color == torch.tensor([0.25, 0.5, 0.75], **f32)).all())
    st.frame("S", "defer")
    misses = [i for i, f in enumerate(st.model.history) if not f.valid]
    print("misses at frames", misses)
    assert misses                                                       # the script does cross capacities


def test_two_streams_do_not_steer_each_other(pkg, dev, monkeypatch):
    """The wide sequence on one stream interleaved with sparse frames on another: the second stream never leaves the
    keyed narrow route, and its trace is the model's run on its own frames alone."""
    R = pkg.rasterizer
    spy = _Spy(R.lib, dev)
    monkeypatch.setattr(R, "lib", spy)
    streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    torch.cuda.synchronize(dev)
    sts = []
    try:
        for s in streams:
            with torch.cuda.stream(s):
                sts.append(_Stream(pkg, dev, spy))
        a, b = sts
        assert a.key != b.key
        script = ["S", "W", "W", "S", "S", "R6", "R6", "W", "S"]
        for i, name in enumerate(script):
            with torch.cuda.stream(streams[0]):
                a.frame(name, "defer" if i % 2 else "block")
            with torch.cuda.stream(streams[1]):
                b.frame("S", "block" if i % 2 else "defer")
        assert a.model.wide > 0 and b.model.wide == 0 and R._wide_depth.get(b.key, 0) == 0
        assert all(f.calls == (M.PROJECT_KEYED, M.KEYED) and f.valid for f in b.model.history[1:])
        assert R._workspaces[(a.key, "n")].data_ptr() != R._workspaces[(b.key, "n")].data_ptr()
    finally:
        torch.cuda.synchronize(dev)
        for st in sts:
            st.restore()                                                # (new streams: nothing to put back)
            R._wide_depth.pop(st.key, None)


# --------------------------------------------------------------------------------------
# the C ABI's contract: a keyed projection must be consumed by a narrow sort (include/cugs_hip.h)
# --------------------------------------------------------------------------------------
def test_abi_keyed_projection_must_be_consumed_by_a_narrow_sort(pkg, dev):
    """The four calls a host could make: keyed projection of an out-of-range view, a *_wide sort (which neither reads nor
    clears the workspace's range flag), keyed projection of an in-range view, cugs_sort_pairs_predicted_keyed - which
    reports the documented -1 although the view is in range; the general route then sorts it correctly, and with the
    flag consumed the same keyed pair is valid."""
    R, lib = pkg.rasterizer, pkg.rasterizer.lib
    S, Wd = scene("S"), scene("W")
    n, w, h = S["n"], 640, 360
    cap = _cap(S["pairs"])
    ms, mw = pkg.scene.to_model(S["arrays"], dev), pkg.scene.to_model(Wd["arrays"], dev)
    i32 = dict(dtype=torch.int32, device=dev)
    ws = torch.zeros(int(lib.cugs_sort_workspace_bytes(n)), dtype=torch.uint8, device=dev)     # a workspace of its own
    wp = torch.empty(int(lib.cugs_sort_pair_workspace_bytes(cap)), dtype=torch.uint8, device=dev)
    st = R._stream(torch.device(dev))
    ptr = R._ptr

    def project_keyed(m, sc):
        p = dict(means=torch.empty((n, 2), device=dev), depths=torch.empty((n,), device=dev),
                 cov=torch.empty((n, 3), device=dev), radii=torch.empty((n,), **i32), tiles=torch.empty((n,), **i32),
                 opa=torch.empty((n,), device=dev), rgb=torch.empty((n, 3), device=dev),
                 packed=torch.empty((n, pkg._lib.PACKED_STRIDE), device=dev))
        cam = sc["cam"].to_abi()
        R.check(lib.cugs_project_forward_keyed(n, int(m.sh_coeffs.shape[2]), DEG, ptr(m.positions), ptr(m.rotations),
                                               ptr(m.scales), ptr(m.opacities), ptr(m.sh_coeffs), C.byref(cam), 1.0,
                                               ptr(p["means"]), ptr(p["depths"]), ptr(p["cov"]), ptr(p["radii"]),
                                               ptr(p["tiles"]), ptr(p["opa"]), ptr(p["rgb"]), ptr(p["packed"]),
                                               C.c_void_p(0), ptr(ws), ws.numel(), st), "cugs_project_forward_keyed")
        return p

    def predicted(entry, p):
        vals, ranges = torch.empty((cap,), **i32), torch.empty((40 * 23, 2), **i32)
        total = torch.zeros(1, dtype=torch.int64).pin_memory()
        R.check(entry(n, cap, ptr(p["means"]), ptr(p["depths"]), ptr(p["radii"]), ptr(p["tiles"]), w, h, ptr(ws),
                      ws.numel(), ptr(wp), wp.numel(), C.c_void_p(0), ptr(vals), ptr(ranges),
                      C.cast(total.data_ptr(), C.POINTER(C.c_int64)), st), "predicted sort")
        torch.cuda.synchronize(dev)
        return int(total[0]), vals, ranges

    def assert_oracle(count, vals, ranges, ref):
        assert count == ref["total_pairs"]
        assert np.array_equal(np_(vals[:count]), ref["values"]) and np.array_equal(np_(ranges), ref["tile_ranges"])

    flag = lambda: int(ws[24:28].view(torch.int32).item())
    pw = project_keyed(mw, Wd)                                         # 1: keyed projection, out of range
    assert flag() != 0
    assert_oracle(*predicted(lib.cugs_sort_pairs_predicted_wide, pw), Wd["ref"])     # 2: the general route, correct ...
    assert flag() != 0                                                 # ... and the flag is still up
    ps = project_keyed(ms, S)                                          # 3: keyed projection, in range
    count, _, _ = predicted(lib.cugs_sort_pairs_predicted_keyed, ps)   # 4: the documented -1
    assert count == -1 and flag() == 0
    assert_oracle(*predicted(lib.cugs_sort_pairs_predicted_wide, ps), S["ref"])      # the wide re-sort is correct
    ps = project_keyed(ms, S)                                          # and the contract kept: keyed -> narrow is valid
    assert_oracle(*predicted(lib.cugs_sort_pairs_predicted_keyed, ps), S["ref"])
