// detect_hooks.h -- what the segment producers and the descriptor path (cs_image_batch.h, lines_host.cpp, lsd_host.cpp, lbd_host.cpp) borrow from a
// detector (detect_host.cpp); not in the public header.
#pragma once
#include "../../include/cubeslam_hip.h"
#include "lines_types.h"

namespace cs {
// the detector's resident scratch slots, in the order cs_detector_destroy releases them
enum ScratchSlot { SCRATCH_EDLINES = 0, SCRATCH_LSD, SCRATCH_LBD, N_SCRATCH_SLOTS };
}

extern "C" {
// the producers run on the detector's stream and device
void* cs_internal_detector_stream(cs_detector* d);
int cs_internal_detector_device(cs_detector* d);
// slot `which` (a cs::ScratchSlot) of the detector: its holder makes the scratch on first use; it is freed with the detector through `deleter`
void** cs_internal_detector_scratch_slot(cs_detector* d, int which, void (*deleter)(void*));
// the one lock of the three slots' holders, and the detector's worker pool
void* cs_internal_detector_lines_mutex(cs_detector* d);
void cs_internal_detector_parallel(cs_detector* d, int n, void (*fn)(int, void*), void* ctx);
// (for the producers' image-long items: two threads per granted CPU at most, see cs_detector_create)
void cs_internal_detector_parallel_long(cs_detector* d, int n, void (*fn)(int, void*), void* ctx);
// the descriptor path (lbd_host.cpp): the EDLines producer with the per-segment extras and a hook that runs under the producers' lock while the
// batch's packed maps are resident (lines_host.cpp)
int cs_internal_detect_lines_batch(cs_detector* d, const unsigned char* const* grays, int n_images, int img_w, int img_h, double length_thres, float* const* lines4, int cap,
                                   int* n_lines, cs::LineExtra* const* extra, int (*then)(void* ctx, const unsigned char* d_p3), void* then_ctx);
}
