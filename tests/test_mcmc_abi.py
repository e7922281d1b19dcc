"""N5 (MCMC densification) C ABI without a GPU: every entry is exported and bound, and argument errors come back as
CUGS_EINVAL (-1) while n == 0 is a successful no-op (0), before anything touches the device."""
import ctypes as C

NAMES = ("cugs_mcmc_random_bits", "cugs_mcmc_regularization", "cugs_mcmc_inject_noise",
         "cugs_mcmc_relocate_workspace_bytes", "cugs_mcmc_relocate", "cugs_project_backward_opts",
         "cugs_project_backward_adam_opts")
GONE = ("cugs_project_backward_pose", "cugs_project_backward_adam_pose", "cugs_project_backward_adam_mcmc",
        "cugs_project_backward_adam_mcmc_pose", "cugs_project_backward_adam_sparse",
        "cugs_project_backward_adam_sparse_pose")            # now options of the two entries above


def test_mcmc_symbols_exported_and_bound(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    from cugs_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    for n in GONE:
        assert not hasattr(lib, n), n
        assert n not in _lib.SIGNATURES, n
    assert hasattr(pkg, "MCMCController") and hasattr(pkg, "MCMCConfig") and hasattr(pkg, "MCMCStats")
    assert C.sizeof(_lib.McmcFused) == 40


def test_mcmc_argument_validation(pkg):
    from cugs_amd._lib import AdamFused, Camera, McmcFused, ProjectionOpts, lib
    null = C.c_void_p(0)
    fake = C.c_void_p(0x1000)
    # generator
    assert lib.cugs_mcmc_random_bits(0, 0, 0, 0, -1, null, null) == -1
    assert lib.cugs_mcmc_random_bits(0, 0, 0, 0, 0, null, null) == 0
    assert lib.cugs_mcmc_random_bits(0, 0, 0, 0, 4, null, null) == -1
    # regulariser
    reg = lambda n, o, s, ws, wsb: lib.cugs_mcmc_regularization(n, o, s, 0.01, 0.01, null, null, null, null, null, ws,
                                                                 wsb, null)
    assert reg(-1, null, null, null, 0) == -1
    assert reg(0, null, null, null, 0) == 0
    assert reg(10, null, null, fake, 1 << 20) == -1
    assert reg(10, fake, fake, fake, 16) == -4                              # workspace too small
    assert lib.cugs_mcmc_regularization(10, fake, fake, 0.01, 0.01, fake, null, null, null, null, fake, 1 << 20,
                                        null) == -1                          # a base without an output
    # noise
    assert lib.cugs_mcmc_inject_noise(-1, null, null, null, 1.0, 100.0, 0.995, null, 0, 0, null) == -1
    assert lib.cugs_mcmc_inject_noise(0, null, null, null, 1.0, 100.0, 0.995, null, 0, 0, null) == 0
    assert lib.cugs_mcmc_inject_noise(10, fake, null, fake, 1.0, 100.0, 0.995, null, 0, 0, null) == -1
    # relocation
    assert lib.cugs_mcmc_relocate_workspace_bytes(-1) == 0
    assert lib.cugs_mcmc_relocate_workspace_bytes(1000) > lib.cugs_mcmc_relocate_workspace_bytes(10) > 0
    rel = lambda n, c, p, st, wsb=1 << 20: lib.cugs_mcmc_relocate(n, c, p, p, p, p, p, 0.005, 0.05, 1.0, 0, 0, None,
                                                                  None, fake, wsb, st, null, null)
    assert rel(-1, 16, null, null) == -1
    assert rel(0, 16, null, null) == 0
    assert rel(0, 17, null, null) == -1                                     # bad coefficient count
    assert rel(10, 16, null, fake) == -1                                    # null parameters
    assert rel(10, 16, fake, null) == -1                                    # null statistics
    assert rel(10, 16, fake, fake, 16) == -4
    m5 = (C.c_void_p * 5)(*([0x1000] * 5))
    assert lib.cugs_mcmc_relocate(10, 16, fake, fake, fake, fake, fake, 0.005, 0.05, 1.0, 0, 0, m5, None, fake, 1 << 20,
                                  fake, null, null) == -1                   # m without v
    # fused route
    cam, adam, mc = Camera(), AdamFused(), McmcFused()
    with_mc = ProjectionOpts(mcmc=C.pointer(mc))
    head = lambda n: (n, 16, 3, null, null, null, null, null, null, null, C.byref(cam), 1.0, null)
    pb = lambda n, opts: lib.cugs_project_backward_adam_opts(*head(n), C.byref(adam), null,
                                                             None if opts is None else C.byref(opts), null)
    plain = lambda n, opts: lib.cugs_project_backward_opts(*head(n), *([null] * 11), C.byref(opts), null)
    assert pb(-1, with_mc) == -1
    assert pb(0, with_mc) == 0
    assert pb(10, with_mc) == -1                                            # null pointers with n > 0
    # no options: the dense fused step
    assert pb(0, None) == 0 == lib.cugs_project_backward_adam(*head(0), C.byref(adam), null, null)
    # requests that no kernel serves, refused before anything else is looked at (n == 0 would return 0)
    assert plain(0, with_mc) == -1                                          # MCMC on the entry without the optimizer step
    assert pb(0, ProjectionOpts(mcmc=C.pointer(mc), sparse=1)) == -1        # MCMC steps every Gaussian
    assert plain(0, ProjectionOpts(sparse=1)) == -1                         # sparse on the entry without the optimizer step
