"""Writes a pack file of a subset of a Kinetics frame tree: every frame prepared once (parsed, un-stuffed, its restart
segments found) and stored as x3dhip.jpegstore.FrameStore keeps it, so that training and validation read it back with bulk
reads (frames.StoredKinetics.from_pack) instead of opening every JPEG file on every rank on every start.

    python tools/pack_frames.py --root DIR --anno JSON --labels TXT --subset validate --out val.pack [--val-windows 3]
                                [--index-bits [N]]

--val-windows N stores only the frames the N validation windows of kinetics.Kinetics draw from each video (they are
deterministic: frames.val_window_frames), which is what a validation pack needs.  The store is kept in plain host memory
(jpegstore.NumpyMemory): no GPU is used.  The pack's meta lists, per video: name, label, first id, stored frames, n_frames
and index, the original frame index of every stored frame (null: all of them in order).

--index-bits N also builds every frame's sync index (the decoder state every N bits of scan, 8 bytes each; without a
value: the library's default) and writes it beside the pack as OUT.idx; a store loaded from the pack then decodes in one
pass per frame.  The pack itself is the same bytes with and without it.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "x3d-multigrid_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def pack(root, anno, labels, subset, out, val_windows=None, sample_duration=80, gamma_tau=5, threads=8, chunk_bytes=64 << 20,
         index_bits=None):
    """Returns (videos, frames, bytes of the pack)."""
    import frames
    from x3dhip import jpegstore
    entries = frames.list_annotation(root, anno, labels, subset)
    store = jpegstore.FrameStore("cpu", memory=jpegstore.NumpyMemory(), threads=threads, chunk_bytes=chunk_bytes,
                                 index_bits=index_bits)
    windows = None
    if val_windows is not None:
        windows = dict(gamma_tau=int(gamma_tau), sample_duration=int(sample_duration), crops=int(val_windows))
    meta = frames.fill_store(store, entries, windows)
    meta["subset"] = subset
    store.save(out, meta)
    return len(entries), len(store), os.path.getsize(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", required=True, help="root of the folders of frame_%%05d.jpg")
    ap.add_argument("--anno", required=True, help="Kinetics annotation json of the reference")
    ap.add_argument("--labels", required=True, help="class list, one name per line")
    ap.add_argument("--subset", required=True, help="train, validate or testing")
    ap.add_argument("--out", required=True, help="the pack file to write")
    ap.add_argument("--val-windows", type=int, default=None, help="store only the frames that many validation windows draw")
    ap.add_argument("--sample-duration", type=int, default=80)
    ap.add_argument("--gamma-tau", type=int, default=5)
    ap.add_argument("--threads", type=int, default=8, help="host threads that prepare the frames (1..16)")
    ap.add_argument("--index-bits", type=int, nargs="?", const=True, default=None,
                    help="also write the sync index of that granularity as OUT.idx (no value: the library's default)")
    args = ap.parse_args(argv)
    if args.val_windows is not None and args.val_windows < 2:
        ap.error("--val-windows: the window step divides by crops - 1, so at least 2")
    videos, nframes, nbytes = pack(args.root, args.anno, args.labels, args.subset, args.out, args.val_windows,
                                   args.sample_duration, args.gamma_tau, args.threads, index_bits=args.index_bits)
    print("%s: %d videos, %d frames, %d bytes (%.0f per frame)" % (args.out, videos, nframes, nbytes, nbytes / max(nframes, 1)))
    if args.index_bits is not None:
        print("%s.idx: %d bytes" % (args.out, os.path.getsize(args.out + ".idx")))


if __name__ == "__main__":
    main()
