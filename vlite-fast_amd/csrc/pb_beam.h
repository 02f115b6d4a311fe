// What the beamformer's two files share: pb_beamform.hip (the weights, the row counts and the beam kernels; pb_beamform,
// pb_beamform_proj) and pb_beam_plane.hip (the beams turned into filterbank planes on the device; pb_beam_planes).  The
// state of a beam call, the beam kernels' arguments, and the two parts of the host path that pb_beam_planes runs too:
// beam_check refuses on the host, beam_queue uploads and queues the beams on the device.
#pragma once
#include "pb_job.h"

#define BEAM_MAX_BEAMS 64

struct BeamArgs {
    const float2 *X;       // one stream's spectra [A][S][2][R][4096]
    const float2 *W;       // [nbeam][A][4096] weights; projecting: [nbeam][2][A][4096]
    const int32_t *shift;  // [4096] first row of output sample 0 per channel
    const int32_t *pref;   // [nbeam][T + 1] rows before t that count for the beam (projecting: [T + 1]); nullptr on the raw stream
    float *beams;          // [nbeam][nout][4][4096]
    int32_t *used;         // [nbeam][nout][4096]
    int S, R, T, nbeam, tscr, nout, spc;   // spc: output samples per workgroup
};

struct PB_LOCAL pb_beam_state : PbJob<3> {      // stages: uploads + weights + row counts, beam kernel, copy to the host
    DevBuf<double> par;                  // [2][BEAM_MAX_BEAMS * PB_SPECTRA_MAX_ANT]: delay / 12500, psi
    DevBuf<float> gain;                  // [BEAM_MAX_BEAMS * PB_SPECTRA_MAX_ANT]
    DevBuf<int32_t> shift;               // [4096]
    DevBuf<float2> proj;                 // [2][A][A][4096]; empty for the plain call, as h_proj is
    DevBuf<float2> W;
    DevBuf<float> beams;
    DevBuf<int32_t> used, pref;
    std::vector<double> h_par;
    std::vector<float> h_gain;
    std::vector<int32_t> h_shift;
    PinBuf<float2> h_proj;               // [2][A][A][4096], the device's layout; pinned, so that the matrices' upload
                                         // is a DMA transfer that does not wait for the host
};

// a call's arguments, and what beam_check works out from them
struct BeamCall {
    int stream, nseg, nbeam;
    const double *delay, *psi;
    const float *gain, *proj;      // proj != nullptr: the projecting call
    const int32_t *shift;
    int tscr, nout;
    int T;                         // the batch's rows
    size_t nused, nval, nproj;     // elements of rows_used, of the beams, of proj (complex)
};

// one more upload that a caller of beam_queue wants among the call's own (stage 0)
struct BeamUpload {
    float *dst;
    const float *src;
    size_t n;
};

// everything the two calls refuse, under the name w, on the host: no HIP call
PB_LOCAL int beam_check(pb_handle *h, const std::string &w, bool projecting, BeamCall &c);
// The checked call on its state bs (made here if need be), up to and including the beam kernel and mark 2: the beams
// (want_beams) and the row counts (want_used) lie in bs->beams and bs->used when bs->st has drained.
PB_LOCAL int beam_queue(pb_handle *h, pb_beam_state *&bs, const BeamCall &c, bool want_beams, bool want_used, const BeamUpload *more);
