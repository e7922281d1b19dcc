// driver_io_check: driver_io.hpp on host tensors alone (no GPU, not linked to the library), for tests/test_driver_io.py.
//   driver_io_check camera <in>                        prints the cugs_camera read_camera returns, one value per line
//   driver_io_check copy <in> <out> <dtype> <count>    load_tensor -> write_raw; dtype is f32, i32 or u8
//   driver_io_check as_f32 <in> <out> <count>          load_tensor(int32) -> write_as_f32
#include "driver_io.hpp"

#include <cstring>

int main(int argc, char** argv) {
    if (argc < 3) return 1;
    const std::string mode = argv[1];
    if (mode == "camera") {
        const cugs_camera cam = read_camera(argv[2]);
        for (float v : cam.view) std::printf("%.9g\n", v);
        std::printf("%.9g\n%.9g\n%.9g\n%.9g\n%d\n%d\n", cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height);
        for (float v : cam.cam_center) std::printf("%.9g\n", v);
        return 0;
    }
    if (mode == "copy" && argc == 6) {
        const auto dtype = !std::strcmp(argv[4], "f32") ? torch::kFloat32 : !std::strcmp(argv[4], "i32") ? torch::kInt32 : torch::kUInt8;
        write_raw(argv[3], load_tensor(argv[2], {std::atoll(argv[5])}, dtype));
        return 0;
    }
    if (mode == "as_f32" && argc == 5) {
        write_as_f32(argv[3], load_tensor(argv[2], {std::atoll(argv[4])}, torch::kInt32));
        return 0;
    }
    return 1;
}
