// Stand-alone host check of the image preprocessing plan: built by tests/test_image_processor_cpu.py together with
// csrc/image_processor.hip under -fsanitize=address,undefined on the host side, and run as a program of its own.  It makes a plan and
// fills the coefficient tables for every shape given on the command line ("in_h in_w edge crop resample grid" each), reads every
// table entry back, and prints one checksum a shape.  No GPU call is made; the few dfh:: services the product file takes from api.hip
// are stubbed here.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/difashion_hip.h"
#include "../../difashion_amd/csrc/dfh_common.h"

namespace dfh {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error() { return g_err.c_str(); }
int check_launch(const char*) { return 0; }
void census(int) {}
bool prof_enabled() { return false; }
void prof_open(int, double, double, hipStream_t) {}
void prof_close(hipStream_t) {}
}  // namespace dfh

int main(int argc, char** argv) {
  if ((argc - 1) % 6 != 0 || argc < 7) { std::fprintf(stderr, "usage: in_h in_w edge crop resample grid ...\n"); return 2; }
  for (int i = 1; i + 5 < argc; i += 6) {
    const int in_h = std::atoi(argv[i]), in_w = std::atoi(argv[i + 1]), grid = std::atoi(argv[i + 5]);
    dfh_imgproc_config cfg = {std::atoi(argv[i + 2]), std::atoi(argv[i + 3]), std::atoi(argv[i + 3]), std::atoi(argv[i + 4])};
    dfh_imgproc* p = nullptr;
    if (dfh_imgproc_create(&cfg, in_h, in_w, grid, &p) != 0) { std::printf("refused: %s\n", dfh::last_error()); continue; }
    const size_t bytes = dfh_imgproc_table_bytes(p);
    std::vector<int> buf(bytes / sizeof(int));                       // exactly table_bytes: a write past it is the sanitizer's to find
    if (dfh_imgproc_fill_tables(p, buf.data(), bytes) != 0) { std::printf("fill failed: %s\n", dfh::last_error()); return 1; }
    if (dfh_imgproc_fill_tables(p, buf.data(), bytes - 1) == 0) { std::printf("a short buffer was accepted\n"); return 1; }
    unsigned long sum = 0;
    for (int v : buf) sum = sum * 1000003UL + (unsigned)v;
    std::printf("%d %d %d %d %d %d -> %d x %d top %d left %d ksize %d %d bytes %zu sum %lu\n", in_h, in_w, cfg.shortest_edge,
                cfg.crop_height, cfg.resample, grid, dfh_imgproc_resized_height(p), dfh_imgproc_resized_width(p), dfh_imgproc_crop_top(p),
                dfh_imgproc_crop_left(p), dfh_imgproc_ksize_x(p), dfh_imgproc_ksize_y(p), bytes, sum);
    dfh_imgproc_destroy(p);
  }
  return 0;
}
