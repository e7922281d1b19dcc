// project_backward_pose.hip — the camera-pose gradient (cugs_projection_opts.pose without sparse).  The
// POSE instantiations of k_project_backward live here, in a translation unit of their own (as the MCMC ones do,
// project_backward_mcmc.hip), so that the existing instantiations keep their code.
//
// The reduction behind the launch, and the pose block's checks, are in project_backward_pose_reduce.h.
#include "project_backward_pose_reduce.h"

extern "C" size_t cugs_pose_grad_workspace_bytes(int64_t n) { return pose_workspace_bytes(n); }

int cugs_pb_check_pose(int64_t n, const cugs_pose_grad* pose) { return check_pose(n, pose); }
int cugs_pb_pose_zeros(const cugs_pose_grad* pose, hipStream_t st) { return pose_zeros(pose, st); }

int cugs_pb_launch_pose(const PBCall& c) {
    const int r = c.mcmc ? launch_pb<true, true, true, false>(c)
                : c.adam ? launch_pb<true, false, true, false>(c)
                         : launch_pb<false, false, true, false>(c);
    if (r != 0) return r;
    return pose_reduce(c.n, c.pose_host, c.st);
}
