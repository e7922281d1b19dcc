"""Sparse Adam C ABI without a GPU: the three entry points are exported and bound, and argument
errors come back as CUGS_EINVAL (-1) / CUGS_EALIGN (-2) while an empty model is a successful no-op (0), before
anything touches the device."""
import ctypes as C
import inspect

EINVAL, EALIGN = -1, -2
NAMES = ("cugs_fused_adam_groups_rows", "cugs_project_backward_opts", "cugs_project_backward_adam_opts")
GONE = ("cugs_project_backward_pose", "cugs_project_backward_adam_pose", "cugs_project_backward_adam_mcmc",
        "cugs_project_backward_adam_mcmc_pose", "cugs_project_backward_adam_sparse",
        "cugs_project_backward_adam_sparse_pose")            # now options of the two entries above
FAKE = 0x10000            # 16-byte aligned, never dereferenced: every call below returns before a launch


def test_sparse_symbols_exported_and_bound(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    from cugs_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    for n in GONE:
        assert not hasattr(lib, n), n
        assert n not in _lib.SIGNATURES, n
    assert "visible" in inspect.signature(pkg.FusedAdam.step).parameters
    assert inspect.signature(pkg.render_backward).parameters["sparse_adam"].default is False


def _groups(pkg, n_rows, widths=(3, 48, 1, 3, 4), count=None, ptr=FAKE):
    from cugs_amd._lib import AdamGroup
    count = len(widths) if count is None else count
    groups = (AdamGroup * max(count, 1))()
    for k in range(count):
        w = widths[k % len(widths)]
        groups[k].param = groups[k].grad = groups[k].m = groups[k].v = ptr
        groups[k].n, groups[k].lr = w * n_rows, 1e-3
    elems = (C.c_int32 * max(count, 1))(*[widths[k % len(widths)] for k in range(max(count, 1))])
    return groups, elems


def test_masked_step_argument_validation(pkg):
    from cugs_amd._lib import lib
    step = lambda g, ng, e, radii, n_rows: lib.cugs_fused_adam_groups_rows(g, ng, e, C.c_void_p(radii), n_rows, 0.9, 0.999,
                                                                           1e-15, 10.0, 1000.0, None)
    g, e = _groups(pkg, 10)
    g[2].n += 1                                              # n != row_elems * n_rows
    assert step(g, 5, e, FAKE, 10) == EINVAL
    g, e = _groups(pkg, 10)
    g[1].n -= 48
    assert step(g, 5, e, FAKE, 10) == EINVAL
    for bad in (0, -3):                                      # row_elems <= 0
        g, e = _groups(pkg, 10)
        e[3] = bad
        assert step(g, 5, e, FAKE, 10) == EINVAL
        g[3].n = 0
        assert step(g, 5, e, FAKE, 10) == EINVAL
    g, e = _groups(pkg, 10)
    assert step(g, 5, e, 0, 10) == EINVAL                    # no radii with rows to step
    g, e = _groups(pkg, 10, count=9)
    assert step(g, 9, e, FAKE, 10) == EINVAL                 # more than 8 groups
    assert step(g, -1, e, FAKE, 10) == EINVAL
    g, e = _groups(pkg, 10)
    assert step(g, 5, e, FAKE, -1) == EINVAL
    assert step(None, 5, e, FAKE, 10) == EINVAL and step(g, 5, None, FAKE, 10) == EINVAL
    g[0].m = None                                            # a stepped group without its moments
    assert step(g, 5, e, FAKE, 10) == EINVAL
    # an empty model: nothing to do, with or without radii
    g, e = _groups(pkg, 0)
    assert step(g, 5, e, 0, 0) == 0 and step(g, 5, e, FAKE, 0) == 0
    assert step(None, 0, None, 0, 0) == 0
    # groups without a gradient are skipped (as cugs_fused_adam_groups skips them): nothing is left to launch
    g, e = _groups(pkg, 10)
    for k in range(5):
        g[k].grad = None
        g[k].n = 7                                           # not looked at either
    assert step(g, 5, e, FAKE, 10) == 0


def _fused(pkg, pose):
    from cugs_amd._lib import AdamFused, Camera, PoseGrad, ProjectionOpts, lib
    cam = Camera()

    def call(n=10, c=16, deg=3, model=FAKE, radii=FAKE, gate=FAKE, accum=FAKE, adam="ok", camera=True, pg="ok"):
        a = AdamFused()
        for k in range(5):
            a.m[k] = a.v[k] = FAKE
        adam_p = C.byref(a) if adam == "ok" else None
        args = [n, c, deg] + [C.c_void_p(model)] * 5 + [C.c_void_p(radii), C.c_void_p(gate),
                                                          C.byref(cam) if camera else None, 1.0, C.c_void_p(accum), adam_p,
                                                          C.c_void_p(FAKE)]
        if not pose:
            return lib.cugs_project_backward_adam_opts(*args, C.byref(ProjectionOpts(sparse=1)), None)
        p = PoseGrad()
        p.dL_dview, p.workspace = FAKE if pg == "ok" else None, FAKE
        p.workspace_bytes = lib.cugs_pose_grad_workspace_bytes(n)
        return lib.cugs_project_backward_adam_opts(*args, C.byref(ProjectionOpts(pose=C.pointer(p), sparse=1)), None)
    return call


def test_fused_sparse_argument_validation(pkg):
    from cugs_amd._lib import lib
    for pose in (False, True):
        call = _fused(pkg, pose)
        assert call(adam=None) == EINVAL                     # null adam_host
        assert call(adam=None, n=0) == EINVAL
        assert call(radii=0) == EINVAL                       # null radii
        assert call(accum=0) == EINVAL                       # null grad_accum
        assert call(accum=FAKE + 4) == EALIGN                # misaligned grad_accum, as the dense entry point
        assert call(model=0) == EINVAL and call(gate=0) == EINVAL and call(camera=False) == EINVAL
        assert call(n=-1) == EINVAL and call(c=5) == EINVAL and call(deg=4) == EINVAL and call(c=4, deg=2) == EINVAL
        if pose:
            assert call(pg=None) == EINVAL                   # a pose block without dL_dview
        else:
            assert call(n=0, model=0, radii=0, gate=0, accum=0) == 0     # an empty model queues nothing
    # the dense entry point answers the same
    dense = lambda accum: lib.cugs_project_backward_adam(10, 16, 3, *([C.c_void_p(FAKE)] * 7), C.byref(_cam(pkg)), 1.0,
                                                         C.c_void_p(accum), C.byref(_adam(pkg)), None, None)
    assert dense(FAKE + 4) == EALIGN and dense(0) == EINVAL


def _cam(pkg):
    from cugs_amd._lib import Camera
    return Camera()


def _adam(pkg):
    from cugs_amd._lib import AdamFused
    a = AdamFused()
    for k in range(5):
        a.m[k] = a.v[k] = FAKE
    return a
