// project_backward_mcmc.hip — the MCMC instantiations of k_project_backward (N5; cugs_projection_opts.mcmc without
// pose), in a translation unit of their own (see project_backward_kernels.h).
#include "project_backward_kernels.h"

int cugs_pb_launch_mcmc(const PBCall& c) { return launch_pb<true, true, false, false>(c); }
