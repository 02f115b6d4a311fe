"""What the tools that replay voltage dumps through a coherence = 1 handle share (correlate.py, beamform.py): their
common arguments and the checks on them, the dump reader, and the batch loop.  A tool keeps what it does with a batch."""
import importlib

import numpy as np

NFFT = 12500


def add_arguments(p):
    p.add_argument("--replay", nargs="+", required=True, help="one dump file per antenna (antenna = position)")
    p.add_argument("--offsets", nargs="+", type=int, default=None, help="samples to advance each antenna by (>= 0)")
    p.add_argument("--stream", choices=("raw", "kur"), default="raw")
    p.add_argument("--seconds", type=int, default=0, help="stop after this many seconds (0 = all)")
    p.add_argument("--rows-per-seg", type=int, default=1024, help="FFT rows per segment of the handle (a multiple of 8)")
    p.add_argument("--max-seg", type=int, default=10, help="segments per batch (1024 x 10 = one second)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("-o", "--output", required=True)


def check_arguments(p, a):
    """p.error unless the files, --offsets (filled in when absent) and the batch's shape make a handle; what a tool
    says about --seconds stands in a message of its own"""
    n = len(a.replay)
    if n > 8:
        p.error("at most 8 antennas")
    if a.offsets is None:
        a.offsets = [0] * n
    if len(a.offsets) != n or min(a.offsets) < 0:
        p.error("--offsets: one value >= 0 per --replay file")
    if a.rows_per_seg <= 0 or a.rows_per_seg % 8 or a.max_seg <= 0:
        p.error("--rows-per-seg must be a positive multiple of 8, --max-seg positive")


class Antenna(object):
    """one dump file as a stream of pol-planar samples, its first `offset` samples dropped"""
    SEC_BYTES = 2 * 25600 * 5032

    def __init__(self, path, offset):
        dada = importlib.import_module("vlite-fast_amd.dada")
        self._vdif = importlib.import_module("vlite-fast_amd.vdif")
        self._ring = dada.FileRing([path])
        if self._ring.next_header() is None:
            raise IOError("%s: no header" % path)
        self._buf = np.empty((2, 0), np.uint8)
        self._drop = offset
        self._eod = False

    def take(self, n):
        """the next n samples per pol, [2][n], or None when the file holds fewer"""
        while self._buf.shape[1] < n and not self._eod:
            raw = self._ring.read(self.SEC_BYTES)
            raw = raw[:len(raw) // (2 * 5032) * (2 * 5032)]
            if not raw:
                self._eod = True
                break
            d = self._vdif.deframe_block(np.frombuffer(raw, np.uint8))
            if self._drop:
                k = min(self._drop, d.shape[1])
                d = d[:, k:]
                self._drop -= k
            self._buf = np.concatenate([self._buf, d], axis=1)
        if self._buf.shape[1] < n:
            return None
        out, self._buf = self._buf[:, :n], self._buf[:, n:]
        return out


def batches(args, prog):
    """Yields (k, handle, stream) for batch k = 0, 1, .. of args.replay once its --max-seg segments of --rows-per-seg
    rows are submitted and processed, until a file holds less than a batch or --seconds (10240 rows each) are covered;
    stream is the library's number of args.stream.  No batch at all ends the tool `prog`."""
    lp = importlib.import_module("vlite-fast_amd.libpb")
    R, S = args.rows_per_seg, args.max_seg
    stream = lp.CORR_KUR if args.stream == "kur" else lp.CORR_RAW
    ants = [Antenna(p, o) for p, o in zip(args.replay, args.offsets)]
    max_batches = -(-args.seconds * 10240 // (S * R)) if args.seconds else 0
    k = 0
    with lp.PbHandle(device=args.device, nant=len(ants), nbit=8, npol=2, rfi_mode=2 if stream else 0, rows_per_seg=R,
                     max_seg=S, coherence=True) as h:
        while not max_batches or k < max_batches:
            blocks = [a.take(S * R * NFFT) for a in ants]
            if any(b is None for b in blocks):
                break
            for ant, b in enumerate(blocks):
                for s in range(S):
                    h.submit_planar(ant, s, b[0, s * R * NFFT:(s + 1) * R * NFFT], b[1, s * R * NFFT:(s + 1) * R * NFFT])
            h.process(S)
            yield k, h, stream
            k += 1
    if k == 0:
        raise SystemExit("%s: the files hold less than one batch of %d rows" % (prog, S * R))
