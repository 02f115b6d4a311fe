#include "second_reader.h"

#include <cstring>

namespace host {

SecondReader::SecondReader(ReadRing *ring, const uint8_t *first, size_t sec_bytes, Log &log)
    : ring(ring), sec_bytes(sec_bytes), log(log), carry(first, first + VD_FRM), current_sec(unpack_header(first).second)
{
}

bool SecondReader::fill(uint8_t *block, size_t &have, VH &next)
{
    have = carry.size();
    memcpy(block, carry.data(), have);
    carry.clear();
    boundary.clear();
    bool eod = false;
    while (boundary.empty() && !eod) {
        if (have < sec_bytes) {
            int64_t got = ring->read(block + have, sec_bytes - have);
            if (got < 0) got = 0;
            if (got % VD_FRM) {
                log.line(false, "Packet size=%d, expected %d.  Aborting this observation.", (int)(got % VD_FRM), (int)VD_FRM);
                got -= got % VD_FRM;
                eod = true;
            } else if ((size_t)got < sec_bytes - have) {
                eod = true;
            }
            have += (size_t)got;
        } else {
            uint8_t nxt[VD_FRM];   // block full and all of this second: the next frame decides
            const int64_t n = ring->read(nxt, VD_FRM);
            if (n != (int64_t)VD_FRM) {
                if (n > 0) log.line(false, "Packet size=%d, expected %d.  Aborting this observation.", (int)n, (int)VD_FRM);
                eod = true;
                break;
            }
            if (unpack_header(nxt).second != current_sec) boundary.assign(nxt, nxt + VD_FRM);
            continue;              // (a duplicate frame of this second: dropped)
        }
        const size_t nfr = have / VD_FRM;
        size_t cut = nfr;
        for (size_t f = 0; f < nfr; ++f) {
            uint32_t w0;
            memcpy(&w0, block + f * VD_FRM, 4);
            if ((int64_t)(w0 & 0x3FFFFFFF) != current_sec) {
                cut = f;
                break;
            }
        }
        if (cut < nfr) {
            boundary.assign(block + cut * VD_FRM, block + have);
            // what follows the cut is not this second's: hide it from the device-side frame index
            for (size_t f = cut; f < nfr; ++f) block[f * VD_FRM + 3] |= 0x80;   // VDIF invalid-data bit
            have = cut * VD_FRM;
        }
    }
    if (boundary.empty()) return false;
    next = unpack_header(boundary.data());
    return true;
}

void SecondReader::seal(uint8_t *block, size_t have)
{
    for (size_t o = have; o + VD_FRM <= sec_bytes; o += VD_FRM) block[o + 3] |= 0x80;
}

void SecondReader::advance()
{
    current_sec = unpack_header(boundary.data()).second;
    carry.swap(boundary);
}

}   // namespace host
