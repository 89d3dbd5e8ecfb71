// detect_hooks.h -- what the segment producers (lines_host.cpp, lsd_host.cpp) borrow from a detector (detect_host.cpp); not in the public header.
#pragma once
#include "../../include/cubeslam_hip.h"
#include "lines_types.h"

extern "C" {
// the producers run on the detector's stream and device
void* cs_internal_detector_stream(cs_detector* d);
int cs_internal_detector_device(cs_detector* d);
// a producer's scratch slot (freed with the detector through `deleter`), the lock of both, and the detector's worker pool
void** cs_internal_detector_lines_slot(cs_detector* d, void (*deleter)(void*));
void** cs_internal_detector_lsd_slot(cs_detector* d, void (*deleter)(void*));
void* cs_internal_detector_lines_mutex(cs_detector* d);
void cs_internal_detector_parallel(cs_detector* d, int n, void (*fn)(int, void*), void* ctx);
// (for the producers' image-long items: two threads per granted CPU at most, see cs_detector_create)
void cs_internal_detector_parallel_long(cs_detector* d, int n, void (*fn)(int, void*), void* ctx);
// the descriptor path (lbd_host.cpp): its scratch slot, and the EDLines producer with the per-segment extras and a hook that runs under the producer's
// lock while the batch's packed maps are resident (lines_host.cpp)
void** cs_internal_detector_lbd_slot(cs_detector* d, void (*deleter)(void*));
int cs_internal_detect_lines_batch(cs_detector* d, const unsigned char* const* grays, int n_images, int img_w, int img_h, double length_thres, float* const* lines4, int cap,
                                   int* n_lines, cs::LineExtra* const* extra, int (*then)(void* ctx, const unsigned char* d_p3), void* then_ctx);
}
