// cs_chunk.h -- the record of a chunked batch kernel's work table, for host and device: cs_batch_handle.h builds the table (chunk_count,
// chunk_fill), cs_wave.h hands a wavefront its entry (wave_chunk).
#pragma once

namespace cs {

// A wave's work: `count` (1 .. the kernel's width, 64) items of ONE owner (a keyframe pair, a job), from item `first` on (an index into
// the whole batch).  16 bytes, read by scalar loads.
struct Chunk {
  int owner, first, count, pad;
};

}  // namespace cs
