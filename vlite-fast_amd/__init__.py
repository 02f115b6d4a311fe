"""vlite-fast_amd: MI355X-native VLITE-Fast baseband -> filterbank front end.

The directory name carries a hyphen (it mirrors the reference's name), so import it with
    importlib.import_module("vlite-fast_amd")      or      import vlite_fast_amd
(the latter is a two-line alias module at the repository root).

Only the hot path of the reference's process_baseband executable lives here:
  csrc/            hand-written gfx950 HIP kernels + the C ABI (include/pb_hip.h)
  libpb.py         ctypes binding of libpb_hip.so (fails loudly if it is missing)
  vdif.py          VDIF frames and psrdada-style ASCII headers (the input contract)
  sigproc.py       SIGPROC .fil header / file writer (the output contract)
  process_baseband.py   the executable's host side, same command-line flags
  genbase.py       genbase-style synthetic baseband (test-side producer)
  coadd.py         incoherent antenna sum across GPUs (torch.distributed / RCCL)
  search.py        dedispersion + boxcar search on the filterbank (stands where heimdall stands): the entry and the
                   public name; its command line, file writers, open_search and main
  searcher.py      Searcher, the ctypes surface of pb_search_*
  gulp.py          GulpSearch, the search over a stream in gulps
  candidates.py    the host's grouping of points into candidates, the candidate line, the TCP leg to the coincidencer
  triggers.py      trigger_t wire format towards the voltage dumper
  correlate.py     visibilities and lag delays of a set of antennas' voltage dumps (pb_correlate*)
  localise.py      fine delays and a sky position from those visibilities (pb_imager_*)
  beamform.py      coherent beams of those antennas at such delays, beside their incoherent sum (pb_beamform); --search / --fil: the
                   beams as planes that stay on the GPU, searched there and written as .fil (pb_beam_planes)
  nulling.py       per-pol, per-channel projectors that take interferers out of those beams (pb_beamform_proj)
  replay_batches.py  what those two tools share: their common arguments, the dump reader, the batch loop over a handle
"""
__version__ = "0.1"
