"""cugs_project_backward_opts / cugs_project_backward_adam_opts without a GPU: no options (NULL or an all-zero block)
answer what the entries without options answer, and a request no kernel serves is CUGS_EINVAL before any other check.
Every call returns before a launch: the pointers are fake."""
import ctypes as C

EINVAL, EALIGN = -1, -2
FAKE = 0x10000            # 16-byte aligned, never dereferenced


def _calls(pkg):
    """(plain, fused, legacy_plain, legacy_fused): callables (n, accum, opts) -> code; opts is a ProjectionOpts or None."""
    from cugs_amd._lib import AdamFused, Camera, lib
    cam, adam = Camera(), AdamFused()
    for k in range(5):
        adam.m[k] = adam.v[k] = FAKE
    P = C.c_void_p
    ref = lambda o: None if o is None else C.byref(o)
    head = lambda n, accum: (n, 16, 3, *([P(FAKE)] * 7), C.byref(cam), 1.0, P(accum))
    tail_plain = (*([None] * 4), *([P(FAKE)] * 5), None, None)
    tail_fused = (C.byref(adam), None)
    return (lambda n, accum, o: lib.cugs_project_backward_opts(*head(n, accum), *tail_plain, ref(o), None),
            lambda n, accum, o: lib.cugs_project_backward_adam_opts(*head(n, accum), *tail_fused, ref(o), None),
            lambda n, accum: lib.cugs_project_backward(*head(n, accum), *tail_plain, None),
            lambda n, accum: lib.cugs_project_backward_adam(*head(n, accum), *tail_fused, None))


def test_no_options_is_the_entry_without_options(pkg):
    from cugs_amd._lib import ProjectionOpts
    assert C.sizeof(ProjectionOpts) == 24
    plain, fused, legacy_plain, legacy_fused = _calls(pkg)
    for entry, legacy in ((plain, legacy_plain), (fused, legacy_fused)):
        for opts in (None, ProjectionOpts()):
            assert entry(10, FAKE + 4, opts) == legacy(10, FAKE + 4) == EALIGN      # misaligned grad_accum
            assert entry(-1, FAKE, opts) == legacy(-1, FAKE) == EINVAL
            assert entry(0, FAKE, opts) == legacy(0, FAKE) == 0                     # n == 0: nothing queued


def test_invalid_requests_are_refused_before_any_other_check(pkg):
    from cugs_amd._lib import McmcFused, ProjectionOpts
    plain, fused, _, _ = _calls(pkg)
    mc = McmcFused()
    invalid = ((plain, ProjectionOpts(mcmc=C.pointer(mc))),               # MCMC without the optimizer step
               (plain, ProjectionOpts(sparse=1)),                         # sparse without the optimizer step
               (fused, ProjectionOpts(mcmc=C.pointer(mc), sparse=1)))     # MCMC steps every Gaussian
    for entry, opts in invalid:
        assert entry(10, FAKE + 4, opts) == EINVAL        # not CUGS_EALIGN: the request is looked at first
        assert entry(0, FAKE, opts) == EINVAL             # not the n == 0 success either
    # each option alone on the fused entry is a valid request: the next check answers
    for opts in (ProjectionOpts(mcmc=C.pointer(mc)), ProjectionOpts(sparse=1)):
        assert fused(10, FAKE + 4, opts) == EALIGN and fused(0, FAKE, opts) == 0
