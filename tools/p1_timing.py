"""Dev tool (GPU box): per-phase cycles of k_bp_bin on the bench workload (variant build `timing`: csrc/dbg.hpp): cycles of thread 0
of every workgroup between the phase marks, averaged over the workgroups."""
import os, sys, ctypes
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dfu3d_amd import synth, _lib
from dfu3d_amd.engine import PseudoBoxEngine
from dfu3d_amd.params import Params
dev = torch.device("cuda", 0)
L = _lib.load_variant("timing")
_lib._LIB = L          # this process drives the timing build through the ordinary engine
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
params = Params()
H, W, M, CAMS, N_PTS = 900, 1600, 8, 6, 34720
scenes = [synth.make_scene(f, H=H, W=W, M=M, cams=CAMS, dense=True, device=dev, k_min=30, k_max=40) for f in range(frames)]
batch = synth.to_view_batch(scenes, params, dev, dense=True, frame_ids=list(range(frames)))
batch.pack_masks()
del scenes
eng = PseudoBoxEngine(params, H, W, M, N_PTS, views_per_chunk=frames * CAMS, dense=True, cap_vox=1 << 18,
                      pool_per_view=1 << 17, device=dev, lanes=1, chain=True)
L.dfu3d_debug_timing_pixel.restype = ctypes.c_int
out = (ctypes.c_ulonglong * 32)()
eng.run(batch); torch.cuda.synchronize()
L.dfu3d_debug_timing_pixel(out, 1)
eng.run(batch); torch.cuda.synchronize()
L.dfu3d_debug_timing_pixel(out, 1)
v = list(out)
# slots: 0-7 cycles of the phases, 8 workgroups, 9 / 10 workgroups that left at the exit (no live pixel) and their cycles from
# entry to exit, 11 workgroups with live pixels of which none is kept or undecided (they have no exit of their own), 12 cycles
# from entry to end of the workgroups that went on
wg = max(v[8], 1)
n1, n2 = v[9], v[11]
live = max(v[8] - n1, 1)
names = ["set-up, depth loads, vote + barrier", "window reset, classification", "origin reduction + barrier", "run merging + LDS atomics",
         "barrier", "flush (global atomics issued)", "barrier", "bit-map flush"]
print("k_bp_bin: %d workgroups (thread 0's cycles)" % v[8])
print("  exit (no live pixel):         %8d workgroups  %5.1f %%  %7.0f cycles each" % (n1, 100.0 * n1 / wg, v[10] / max(n1, 1)))
print("  going on:                     %8d workgroups  %5.1f %%  %7.0f cycles each" % (v[8] - n1, 100.0 * (v[8] - n1) / wg, v[12] / live))
print("    live, nothing kept:         %8d workgroups  %5.1f %%  (no exit of their own)" % (n2, 100.0 * n2 / wg))
# the first phase is every workgroup's, the others only those of the workgroups that went on: each average over its own
print("  phase                                  cycles per workgroup that ran it   share of all cycles")
tot = max(sum(v[:8]), 1)
for i, nm in enumerate(names):
    print("  %-36s %9.0f  (%6d workgroups)  %5.1f %%" % (nm, v[i] / (wg if i == 0 else live), v[8] if i == 0 else v[8] - n1, 100.0 * v[i] / tot))
