// k_detect2's workgroups in dispatch order: which (channel group, stream) block b of a launch's 1-D grid takes.
// Plain C / C++, host and device (tests/test_d2_block_map_cpu.py builds it on the host).
//
// One stream (RFI modes 0, 1): block b is channel group b.
// Two streams (RFI mode 2): the excised stream's 128 workgroups first, then the raw stream's -- the long-lived kind
// before the short-lived one (why, and what else was measured: profiles/r09_notes.md).
// A PLACEMENT CHOICE ONLY: nothing waits for, polls or signals another workgroup, and every result is the same wherever
// and whenever a block runs.
#ifndef D2_BLOCK_MAP_H
#define D2_BLOCK_MAP_H

#ifdef __HIPCC__
#define D2_MAP_FN __host__ __device__ static inline
#else
#define D2_MAP_FN static inline
#endif

#define D2_NCG 128                 // channel groups of 32 channels

typedef struct {
    int cg, stream;                // channel group; 0 raw, 1 excised (always 0 with one stream)
} d2_block;

D2_MAP_FN d2_block d2_block_map(int b, int nstream)
{
    d2_block m;
    m.cg = b % D2_NCG;
    m.stream = nstream == 2 ? 1 - b / D2_NCG : 0;
    return m;
}

#endif
