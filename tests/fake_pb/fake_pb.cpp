// Stand-in for libpb_hip.so under the native host program (vlite-fast_amd/csrc/process_baseband), for
// tests/test_native_host_cpu.py: exactly the entry points of include/pb_hip.h that the program calls, no HIP,
// everything in host memory.  Linked in place of the library (make -C vlite-fast_amd/csrc host-standin), not injected.
//
// pb_submit_vdif_at deframes on the host by the placement rule of pb_stage.hip / vdif.deframe_block.  The "filterbank
// bytes" of a segment are a FOLD of its samples, so that every sample of the second and its position reach the output
// (a prefix of the samples would cover the first few frames only):
//     out[seg][j] = sum over i in [0, seg_samples), i % trim == j, of (2 * (i / trim) + 1) * x[seg * seg_samples + i]
// mod 256, for j in [0, trim), trim = code_bytes_per_seg.  The weights are odd, so changing any one sample changes the
// output; moving a frame changes both the weights and the columns its samples fall in.  Stream 0 (raw) folds the
// samples of pol 0 (VDIF thread 0), stream 1 (excised) those of pol 1.  FoldHandle in the test restates it in numpy.
//
// $FAKE_PB_TRACE names a file that gets one line per reset / submit / process / fetch call, in order.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pb_hip.h"

struct pb_handle {
    pb_config cfg;
    int cur = 0;
    size_t seg_samples = 0, trim = 0;
    std::vector<std::vector<uint8_t>> staged, done;   // [set]: [2 pols][max_seg * seg_samples]
    std::vector<std::vector<uint8_t>> codes;          // [2 * set + stream]: [max_seg][trim]
    std::vector<char> unfetched;                      // [set]: processed, output not looked at yet
    std::string err;
    FILE *trace = nullptr;
};

static std::string g_err;

static int fail(pb_handle *h, int code, const char *msg)
{
    h->err = msg;
    return code;
}

extern "C" {

void pb_config_default(pb_config *c)
{
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c;
    c->nant = 1;
    c->nbit = 2;
    c->npol = 1;
    c->rfi_mode = 2;
    c->taps = 1;
    c->rows_per_seg = 1024;
    c->max_seg = 1;
    c->nsets = 1;
}

int pb_create(const pb_config *c, pb_handle **out)
{
    if (c->rows_per_seg <= 0 || c->rows_per_seg % 8 || c->max_seg < 1 || c->nsets < 1) {
        g_err = "fake pb_create: bad geometry";
        return PB_EINVAL;
    }
    pb_handle *h = new pb_handle;
    h->cfg = *c;
    h->seg_samples = (size_t)c->rows_per_seg * PB_NFFT;
    h->trim = (size_t)(c->coherence ? 4 : c->npol) * (c->rows_per_seg / PB_NSCRUNCH) * PB_NCHANOUT * c->nbit / 8;
    h->staged.resize(c->nsets);
    h->done.resize(c->nsets);
    h->codes.resize(2 * (size_t)c->nsets);
    h->unfetched.assign(c->nsets, 0);
    if (const char *t = getenv("FAKE_PB_TRACE")) h->trace = fopen(t, "a");
    *out = h;
    return PB_OK;
}

void pb_destroy(pb_handle *h)
{
    if (h && h->trace) fclose(h->trace);
    delete h;
}

const char *pb_last_error(const pb_handle *h) { return h ? h->err.c_str() : g_err.c_str(); }

int pb_query(const pb_handle *h, pb_sizes *o)
{
    memset(o, 0, sizeof *o);
    o->seg_samples_per_pol = h->seg_samples;
    o->input_bytes_per_seg = 2 * h->seg_samples;
    o->code_bytes_per_seg = h->trim;
    o->rows_per_seg = h->cfg.rows_per_seg;
    return PB_OK;
}

void *pb_host_alloc(size_t n) { return malloc(n ? n : 1); }
void pb_host_free(void *p) { free(p); }
int pb_sync(pb_handle *) { return PB_OK; }
int pb_profile(pb_handle *, int) { return PB_OK; }

int pb_get_timers(pb_handle *, pb_timers *t, int)
{
    memset(t, 0, sizeof *t);
    return PB_OK;
}

int pb_reset_history(pb_handle *h, int ant)
{
    if (h->trace) fprintf(h->trace, "reset %d\n", ant);
    return PB_OK;
}

int pb_select_set(pb_handle *h, int set)
{
    if (set < 0 || set >= h->cfg.nsets) return fail(h, PB_EINVAL, "fake pb_select_set: no such set");
    h->cur = set;
    return PB_OK;
}

int pb_submit_vdif_at(pb_handle *h, int, int seg0, const uint8_t *block, size_t nbytes, int64_t sec0, int64_t fr0)
{
    if (h->unfetched[h->cur]) return fail(h, PB_ESTATE, "fake pb_submit_vdif_at: buffer set refilled before its output was fetched");
    if (nbytes == 0 || nbytes % (2 * PB_VDIF_FRAME)) return fail(h, PB_EINVAL, "fake pb_submit_vdif_at: block is not a whole number of frame pairs");
    const size_t nslots = nbytes / PB_VDIF_FRAME, nfr = nslots / 2;
    if (seg0 != 0 || nfr * PB_VDIF_DATA != (size_t)h->cfg.max_seg * h->seg_samples)
        return fail(h, PB_EINVAL, "fake pb_submit_vdif_at: block does not fill segments [0, max_seg)");
    std::vector<uint8_t> &d = h->staged[h->cur];
    d.assign(2 * nfr * PB_VDIF_DATA, 0);              // missing frames stay zero
    for (size_t i = 0; i < nslots; ++i) {
        const uint8_t *p = block + i * PB_VDIF_FRAME;
        uint32_t w0, w1, w3;
        memcpy(&w0, p, 4);
        memcpy(&w1, p + 4, 4);
        memcpy(&w3, p + 12, 4);
        if (w0 & 0x80000000u) continue;               // invalid-data bit
        const int thread = ((w3 >> 16) & 0x3ff) != 0;
        const int64_t rel = ((int64_t)(w0 & 0x3fffffff) - sec0) * PB_FRAMES_PER_SEC + (int64_t)(w1 & 0xffffff) - fr0;
        if (rel < 0 || rel >= (int64_t)nfr) continue;
        memcpy(d.data() + ((size_t)thread * nfr + (size_t)rel) * PB_VDIF_DATA, p + (PB_VDIF_FRAME - PB_VDIF_DATA), PB_VDIF_DATA);
    }
    if (h->trace) fprintf(h->trace, "submit %d %lld %lld\n", h->cur, (long long)sec0, (long long)fr0);
    return PB_OK;
}

int pb_process(pb_handle *h, int nseg, int inject_now)
{
    if (nseg != h->cfg.max_seg || h->staged[h->cur].empty()) return fail(h, PB_ESTATE, "fake pb_process: nothing staged");
    h->done[h->cur].swap(h->staged[h->cur]);
    h->staged[h->cur].clear();
    h->unfetched[h->cur] = 1;
    if (h->trace) fprintf(h->trace, "process %d %d %d\n", h->cur, nseg, inject_now);
    return PB_OK;
}

int pb_fetch_ptr(pb_handle *h, int, int stream, const uint8_t **out)
{
    const std::vector<uint8_t> &d = h->done[h->cur];
    if (d.empty() || stream < 0 || stream > 1) return fail(h, PB_ESTATE, "fake pb_fetch_ptr: nothing processed on this set");
    const size_t S = (size_t)h->cfg.max_seg, n = h->seg_samples, trim = h->trim;
    std::vector<uint8_t> &c = h->codes[2 * (size_t)h->cur + stream];
    c.assign(S * trim, 0);
    const uint8_t *x = d.data() + (size_t)stream * S * n;
    for (size_t s = 0; s < S; ++s)
        for (size_t i = 0; i < n; ++i)                // the fold of the header comment
            c[s * trim + i % trim] = (uint8_t)(c[s * trim + i % trim] + (2 * (i / trim) + 1) * x[s * n + i]);
    h->unfetched[h->cur] = 0;
    if (h->trace) fprintf(h->trace, "fetch %d %d\n", h->cur, stream);
    *out = c.data();
    return PB_OK;
}

}   // extern "C"
