// project_backward_sparse.hip — the visibility-restricted fused optimizer step (DESIGN.md 4.20;
// cugs_projection_opts.sparse, with or without pose).  The SPARSE instantiations of k_project_backward live here, in a
// translation unit of their own (as the MCMC and POSE ones do), so that the existing instantiations keep their code.
// Same routes as the dense fused step: aligned or not, C = 1, 4, 9, 16, factor tile for aligned degree-3 storage.
#include "project_backward_pose_reduce.h"

int cugs_pb_launch_sparse(const PBCall& c) {
    if (!c.pose_host) return launch_pb<true, false, false, true>(c);
    const int r = launch_pb<true, false, true, true>(c);
    if (r != 0) return r;
    return pose_reduce(c.n, c.pose_host, c.st);
}
