// The frames of one observation, one second at a time: SecondReader of vlite-fast_amd/process_baseband.py, same
// operations, same names, same steps (src/process_baseband.cu:1015-1067 of the reference).
#ifndef PB_HOST_SECOND_READER_H
#define PB_HOST_SECOND_READER_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "formats.h"
#include "log.h"
#include "rings.h"

namespace host {

// Frames are placed by their own headers (thread id, frame number: :1017-1034), a second is closed by the
// first frame of another second (:1019, :1058) and dispatched only then, and a frame that never arrives
// leaves zeros.  The frames of one second are gathered in a page-locked block in bulk; when frames were
// dropped the block swallows the head of the next second, which is carried over, so that the stream
// re-aligns at once.
struct SecondReader {
    ReadRing *ring;
    const size_t sec_bytes;
    Log &log;
    std::vector<uint8_t> carry;      // frames of the second being assembled that have been read already
    std::vector<uint8_t> boundary;   // bytes (>= one frame) of the next second, already read
    int64_t current_sec;
    SecondReader(ReadRing *ring, const uint8_t *first, size_t sec_bytes, Log &log);
    // Assemble second `current_sec` in `block`.  -> true: `have` = bytes of this second in the block (frames of other
    // seconds behind them are marked invalid), `next` = header of the first frame of the next second; false at the end
    // of data (the last, partial or whole, second is dropped)
    bool fill(uint8_t *block, size_t &have, VH &next);
    // frames were dropped: whatever an earlier second left in the tail of the block is not data
    void seal(uint8_t *block, size_t have);
    // the second in the block has been handed on: the next one starts with what was read beyond it
    void advance();
};

}   // namespace host

#endif
