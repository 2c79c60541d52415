// Dumps the two address maps of csrc/wino_s3_lds_map.h for tests/test_wino_s3_lds_map.py (host compiler only):
//   const <kS3K> <kS3Pairs> <kS3Plane> <kS3Stage>
//   st <tid> <byte offset of the thread's 8 staged bytes in a (product, plane) block>       tid = 0 .. 255
//   rd <pair group> <lane> <byte offset of the lane's 16-byte A fragment in the block>      lane = 0 .. 63
#include <cstdio>

#include "wino_s3_lds_map.h"

int main() {
    using namespace xvec::wino;
    std::printf("const %d %d %d %d\n", kS3K, kS3Pairs, kS3Plane, kS3Stage);
    for (int tid = 0; tid < 256; ++tid) std::printf("st %d %d\n", tid, s3_st_off(tid));
    for (int g = 0; g < 2; ++g)
        for (int lane = 0; lane < 64; ++lane) std::printf("rd %d %d %d\n", g, lane, s3_a_rd(lane, g));
    return 0;
}
