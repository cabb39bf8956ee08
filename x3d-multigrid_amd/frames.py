"""Folders of JPEG frames as a data source: the reference's on-disk protocol (kinetics.py:43-51: `frame_%05d.jpg`, 1-based)
read from disk on the host and decoded on the GPU by x3dhip.jpegops.JpegDecoder (libx3djpeg.so, bit-exact with the PIL
decode of the reference's loader).

FrameFolder      one video: frame count and size from the listing and the first file's header, raw bytes on demand
FolderKinetics   DeviceVideoKinetics' batch / val_batch protocol over frame folders: only the frames a sample draws are
                 decoded, straight into the [T, H, W, 3] tensor ClipPreprocessor consumes
decode_folder    a whole video as uint8 [n, H, W, 3] in HBM (what charades.Charades(videos=...) takes)
StoredVideo      a whole video in HBM as the prepared scans of its JPEG files (x3dhip.jpegstore.FrameStore), about the size
                 of the files: charades.Charades takes it wherever it takes a decoded video and decodes, per batch, the
                 frames the batch draws
StoredKinetics   FolderKinetics' batches, bit for bit, over StoredVideos: the store lives in HBM (tier='device') or in
                 pinned host memory (tier='host', for a set larger than HBM), filled from folders or read from a pack
                 file (FrameStore.save / load; tools/pack_frames.py writes one without a GPU)
"""
import json
import os
import random

import torch

from cycle_batch_sampler import long_cycle_shapes
from kinetics_multigrid import DeviceVideoKinetics

FRAME_NAME = 'frame_{:05d}.jpg'
MIN_FRAMES = 80 + 1          # kinetics.py:124: videos with n_frames <= 81 are skipped


class FrameFolder:
    """One video as the reference stores it: files frame_00001.jpg, frame_00002.jpg, ... without a gap (video_loader stops
    at the first missing file, kinetics.py:43-51).  n_frames and (W, H) come from the listing and the first file's header;
    nothing is decoded.  name: the file name format (the reference's Charades loader has '<video id>-{:06d}.jpg',
    charades.py:47).  entropy: where this video's frames are Huffman decoded ('host' or 'device'), for decode_folder to
    pass on to its decoder; None leaves it to the caller."""

    def __init__(self, path, name=FRAME_NAME, entropy=None):
        from x3dhip.jpegops import read_header
        if entropy not in (None, 'host', 'device'):
            raise ValueError("entropy must be 'host' or 'device' (got %r)" % (entropy,))
        self.path, self.name, self.entropy = path, name, entropy
        names = set(os.listdir(path))
        n = 0
        while name.format(n + 1) in names:
            n += 1
        if n == 0:
            raise ValueError("%s holds no %s" % (path, name.format(1)))
        self.n_frames = n
        self.width, self.height = read_header(self._bytes(0))

    def _bytes(self, i):
        with open(os.path.join(self.path, self.name.format(i + 1)), 'rb') as f:
            return f.read()

    def read(self, indices):
        """The files of the 0-based frames `indices`, as bytes."""
        for i in indices:
            if not 0 <= i < self.n_frames:
                raise ValueError("frame %d outside the %d frames of %s" % (i, self.n_frames, self.path))
        return [self._bytes(i) for i in indices]


def video_names_and_labels(data, subset):
    """get_video_names_and_annotations (kinetics.py:74-95): folder name per video of the subset, and its label string (None
    for 'testing', which has no annotations)."""
    out = []
    for key, value in data.items():
        if value['subset'] != subset:
            continue
        if subset == 'testing':
            out.append(('test/{}'.format(key), None))
        elif subset == 'train':
            seg = value['annotations']['segment']
            label = value['annotations']['label']
            out.append(('{}/{}_{}_{}'.format(label.replace(' ', '_'), key, str(int(seg[0])).zfill(6),
                                             str(int(seg[1])).zfill(6)), label))
        else:
            label = value['annotations']['label']
            out.append(('{}/{}'.format(label.replace(' ', '_'), key), label))
    return out


def class_labels(lines):
    """get_class_labels (kinetics.py:64-71): class index = line number in the label file."""
    return {name: i for i, name in enumerate(lines)}


def list_dataset(root, data, class_to_idx, subset):
    """make_dataset (kinetics.py:98-158) for n_samples_for_each_video == 1: [(FrameFolder, label)], skipping videos whose
    folder is missing or that have n_frames <= 81.  label is -1 where the subset has no annotations."""
    out = []
    for name, label in video_names_and_labels(data, subset):
        path = os.path.join(root, name)
        if not os.path.exists(path):
            continue
        if len(os.listdir(path)) <= MIN_FRAMES:
            continue
        out.append((FrameFolder(path), -1 if label is None else class_to_idx[label]))
    return out


def list_annotation(root, anno_json, labels_txt, subset):
    """list_dataset from paths: anno_json and labels_txt are paths (or an annotation dict and a list of class names).
    ValueError when the subset has no video under root."""
    data = anno_json
    if not isinstance(data, dict):
        with open(anno_json, 'r') as f:
            data = json.load(f)
    lines = labels_txt
    if isinstance(lines, str):
        lines = open(labels_txt).read().splitlines()
    entries = list_dataset(root, data, class_labels(lines), subset)
    if not entries:
        raise ValueError("no video of subset %r under %s" % (subset, root))
    return entries


class FolderKinetics(DeviceVideoKinetics):
    """DeviceVideoKinetics over frame folders instead of decoded videos: same draws (draw_clip_params / val_crop_indices /
    center_crop_box, through the parent's batch and val_batch), same return values.  Per sample only the drawn frames
    are read and decoded, into a [T, H, W, 3] tensor that the clip kernels then index with range(T)."""

    class _Video:
        """What the parent's loops ask of a video: .shape = (n_frames, H, W, 3)."""

        def __init__(self, folder):
            self.folder = folder
            self.shape = (folder.n_frames, folder.height, folder.width, 3)

    def __init__(self, folders, labels, sample_duration=80, gamma_tau=5, crop_size=224, x3d_version='M', rng=None,
                 device='cuda:0', threads=8, entropy='host'):
        from x3dhip.clip_input import ClipPreprocessor
        from x3dhip.jpegops import JpegDecoder
        if len(folders) != len(labels) or not folders:
            raise ValueError("one label per folder, at least one folder")
        self.folders = [f if isinstance(f, FrameFolder) else FrameFolder(f) for f in folders]
        self.videos = [self._Video(f) for f in self.folders]
        self.labels = labels
        self.sample_duration, self.gamma_tau, self.crop_size = sample_duration, gamma_tau, crop_size
        self.long_cycles = long_cycle_shapes(sample_duration, crop_size)
        self.scales = [crop_size / i for i in self.RESIZE[x3d_version]]
        self.rng = rng if rng is not None else random
        self.device = torch.device(device)
        self.decoder = JpegDecoder(self.device, threads=threads, entropy=entropy)
        self._pre = ClipPreprocessor(self.device)

    def pre(self, samples, out=None):
        """The parent hands over (video, params) per sample; decode each sample's frames (one decoder batch for all
        samples), then run the clip kernels on them."""
        files, slots = [], []
        for v, p in samples:
            idx = p["frame_idx"]
            files += v.folder.read(idx)
            slots.append((v, len(idx)))
        decoded, at = [], 0
        same = len({v.shape[1:] for v, _ in slots}) == 1
        if same:                                             # one destination tensor, one job table
            H, W = slots[0][0].shape[1:3]
            buf = torch.empty((len(files), H, W, 3), dtype=torch.uint8, device=self.device)
            self.decoder.decode_into(files, buf)
            for v, T in slots:
                decoded.append(buf[at:at + T])
                at += T
        else:
            bufs = [torch.empty((T, v.shape[1], v.shape[2], 3), dtype=torch.uint8, device=self.device) for v, T in slots]
            self.decoder.decode(files, out=[b[t] for b in bufs for t in range(b.shape[0])])
            decoded = bufs
        clips = [(d, dict(p, frame_idx=list(range(d.shape[0])))) for d, (_, p) in zip(decoded, samples)]
        return self._pre(clips, out=out)

    @classmethod
    def from_annotation(cls, root, anno_json, labels_txt, subset, **kw):
        """The reference's dataset listing (kinetics.py:59-158): anno_json and labels_txt are paths (or an annotation dict
        and a list of class names)."""
        entries = list_annotation(root, anno_json, labels_txt, subset)
        return cls([e[0] for e in entries], [e[1] for e in entries], **kw)


def decode_folder(path, device, threads=8, decoder=None, chunk=256, name=FRAME_NAME, entropy=None):
    """A whole video as uint8 [n_frames, H, W, 3] on `device`.  entropy: 'host' or 'device' Huffman decoding (None: what
    the FrameFolder says, else 'host'); a ready `decoder` keeps its own."""
    from x3dhip.jpegops import JpegDecoder
    folder = path if isinstance(path, FrameFolder) else FrameFolder(path, name, entropy=entropy)
    dec = decoder if decoder is not None else JpegDecoder(device, threads=threads,
                                                          entropy=entropy or folder.entropy or 'host')
    out = torch.empty((folder.n_frames, folder.height, folder.width, 3), dtype=torch.uint8, device=dec.device)
    for s in range(0, folder.n_frames, chunk):
        e = min(folder.n_frames, s + chunk)
        dec.decode_into(folder.read(range(s, e)), out[s:e])
    return out


class StoredVideo:
    """One video in a FrameStore: frames ids[0], ids[1], ... of the store, all of one size.  .shape is what the decoded
    video's would be; .frames(idx) decodes the 0-based frames idx now."""

    def __init__(self, store, ids):
        ids = range(ids.start, ids.stop) if isinstance(ids, range) and ids.step == 1 else ids
        if not isinstance(ids, range) or len(ids) < 1 or ids.start < 0 or ids.stop > len(store):
            raise ValueError("ids must be a non-empty range of frame ids of the store")
        w, h = store.width[ids.start:ids.stop], store.height[ids.start:ids.stop]
        if (w != w[0]).any() or (h != h[0]).any():
            raise ValueError("the frames of a video are of one size")
        self.store, self.ids, self.device = store, ids, store.device
        self.shape = (len(ids), int(h[0]), int(w[0]), 3)

    def frame_ids(self, idx):
        """The store's ids of the 0-based frames idx."""
        n = self.shape[0]
        for i in idx:
            if not 0 <= i < n:
                raise ValueError("frame %d outside the %d frames of the video" % (i, n))
        return [self.ids.start + i for i in idx]

    def frames(self, idx):
        """uint8 [len(idx), H, W, 3] on the store's device."""
        ids = self.frame_ids(list(idx))
        out = torch.empty((len(ids),) + self.shape[1:], dtype=torch.uint8, device=self.device)
        return self.store.decode_into(ids, out)


class WindowedVideo(StoredVideo):
    """A video of which the store holds only some frames (the ones the validation windows draw): .shape is the whole
    video's, index the original 0-based frame index of each stored frame, in the order of ids.  A frame that is not
    stored raises ValueError naming the video."""

    def __init__(self, store, ids, n_frames, index, name=None):
        super().__init__(store, ids)
        index = [int(i) for i in index]
        if len(index) != len(self.ids) or any(not 0 <= i < n_frames for i in index):
            raise ValueError("one original frame index below %d per stored frame" % n_frames)
        self.name = name
        self._at = {orig: k for k, orig in enumerate(index)}
        self.shape = (int(n_frames),) + self.shape[1:]

    def frame_ids(self, idx):
        try:
            return [self.ids.start + self._at[int(i)] for i in idx]
        except KeyError as e:
            raise ValueError("frame %s of video %s is not in the pack (it holds %d of its %d frames)" % (
                e.args[0], self.name, len(self.ids), self.shape[0])) from None


def decode_stored(samples):
    """samples: dicts with 'frames' and 'frame_idx' (as dataops.ClipBatcher takes them).  Every sample whose 'frames' is a
    StoredVideo gets, in place, the uint8 tensor of exactly its frame_idx and frame_idx = range(len): one decode_into per
    store and frame size over all samples (what FolderKinetics.pre does for folders)."""
    groups = {}
    for s in samples:
        v = s["frames"]
        if isinstance(v, StoredVideo):
            groups.setdefault((id(v.store),) + v.shape[1:3], []).append(s)
    for group in groups.values():
        v = group[0]["frames"]
        for s in group:
            n = s["frames"].shape[0]
            if any(not 0 <= i < n for i in s["frame_idx"]):
                raise ValueError("frame index outside the video")
        ids = [i for s in group for i in s["frames"].frame_ids(s["frame_idx"])]
        buf = torch.empty((len(ids),) + v.shape[1:], dtype=torch.uint8, device=v.device)
        v.store.decode_into(ids, buf)
        at = 0
        for s in group:
            T = len(s["frame_idx"])
            s["frames"], s["frame_idx"] = buf[at:at + T], range(T)
            at += T


def val_window_frames(n_frames, gamma_tau, sample_duration, crops):
    """The sorted 0-based frames of a video that the validation windows of kinetics.Kinetics draw (they do not depend on
    anything but these four numbers)."""
    from x3dhip.clip_input import val_crop_indices
    return sorted({int(i) for idx in val_crop_indices(n_frames, gamma_tau, sample_duration, crops) for i in idx})


def fill_store(store, entries, windows=None, chunk=256):
    """Adds the frames of entries ([(FrameFolder, label)]) to the store; windows: dict(gamma_tau=, sample_duration=,
    crops=) to store only the frames the validation windows draw.  Returns the pack meta of the videos: name (the folder
    relative to nothing: its path's last two parts), label, first id, stored frames, n_frames and index (the original
    frame index of every stored frame; None stands for all of them in order)."""
    videos = []
    for folder, label in entries:
        index = None if windows is None else val_window_frames(folder.n_frames, **windows)
        want = list(range(folder.n_frames)) if index is None else index
        first = len(store)
        for s in range(0, len(want), chunk):
            store.add(folder.read(want[s:s + chunk]))
        videos.append(dict(name="/".join(os.path.normpath(folder.path).split(os.sep)[-2:]), label=int(label), first=first,
                           frames=len(want), n_frames=folder.n_frames, index=index))
    return dict(videos=videos, windows=windows)


class StoredKinetics(DeviceVideoKinetics):
    """FolderKinetics over StoredVideos: the same draws from the parent (draw_clip_params / val_crop_indices /
    center_crop_box), so that with equal rng seeds a batch is bit for bit the FolderKinetics batch; per batch the drawn
    frames are decoded from the store by id (decode_stored), then the same clip kernels run."""

    def __init__(self, videos, labels, sample_duration=80, gamma_tau=5, crop_size=224, x3d_version='M', rng=None, meta=None):
        from x3dhip.clip_input import ClipPreprocessor
        if len(videos) != len(labels) or not videos:
            raise ValueError("one label per video, at least one video")
        self.videos, self.labels, self.meta = list(videos), list(labels), meta
        self.store = self.videos[0].store
        self.sample_duration, self.gamma_tau, self.crop_size = sample_duration, gamma_tau, crop_size
        self.long_cycles = long_cycle_shapes(sample_duration, crop_size)
        self.scales = [crop_size / i for i in self.RESIZE[x3d_version]]
        self.rng = rng if rng is not None else random
        self.device = self.store.device
        self._pre = ClipPreprocessor(self.device)

    def pre(self, samples, out=None):
        drawn = [dict(frames=v, frame_idx=list(p["frame_idx"])) for v, p in samples]
        decode_stored(drawn)
        clips = [(d["frames"], dict(p, frame_idx=list(d["frame_idx"]))) for d, (_, p) in zip(drawn, samples)]
        return self._pre(clips, out=out)

    @classmethod
    def from_annotation(cls, root, anno_json, labels_txt, subset, tier='device', device='cuda:0', threads=8,
                        chunk_bytes=None, rank=0, world=1, **kw):
        """The listing of FolderKinetics.from_annotation, its videos i % world == rank read into a FrameStore of `tier`."""
        from x3dhip.jpegstore import FrameStore
        entries = list_annotation(root, anno_json, labels_txt, subset)[rank::world]
        if not entries:
            raise ValueError("rank %d of %d has no video of subset %r under %s" % (rank, world, subset, root))
        store = FrameStore(device, threads=threads, tier=tier, **({} if chunk_bytes is None else dict(chunk_bytes=chunk_bytes)))
        meta = fill_store(store, entries)
        return cls._over(store, meta, [range(v["first"], v["first"] + v["frames"]) for v in meta["videos"]], **kw)

    @classmethod
    def from_pack(cls, path, device='cuda:0', tier='device', rank=0, world=1, chunk_bytes=None, **kw):
        """The videos i % world == rank of a pack file (tools/pack_frames.py, or FrameStore.save with fill_store's meta):
        only their frames are read."""
        from x3dhip.jpegstore import FrameStore
        meta = FrameStore.read_meta(path)
        if not isinstance(meta, dict) or not isinstance(meta.get("videos"), list):
            raise ValueError("%s carries no list of videos" % path)
        mine = meta["videos"][rank::world]
        if not mine:
            raise ValueError("rank %d of %d has no video of %s" % (rank, world, path))
        store, _, id_map = FrameStore.load(path, device, tier=tier, ranges=[range(v["first"], v["first"] + v["frames"])
                                                                            for v in mine],
                                           **({} if chunk_bytes is None else dict(chunk_bytes=chunk_bytes)))
        return cls._over(store, dict(meta, videos=mine), id_map, **kw)

    @classmethod
    def _over(cls, store, meta, ids, **kw):
        videos = [StoredVideo(store, r) if v.get("index") is None else
                  WindowedVideo(store, r, v["n_frames"], v["index"], v["name"]) for v, r in zip(meta["videos"], ids)]
        return cls(videos, [v["label"] for v in meta["videos"]], meta=meta, **kw)


def charades_videos(root, anno, device, threads=8, entropy='host', resident='decoded', chunk_bytes=None, tier='device'):
    """{video id: video} for every video of the annotation dict that has a folder under root: the `videos` argument of
    charades.Charades and the Charades training scripts.  resident='decoded': uint8 [n, H, W, 3], decoded whole.
    resident='compressed': StoredVideo over one FrameStore shared by all videos (chunk_bytes: its arena chunk size),
    decoded batch by batch on the GPU, Huffman decoding included; `entropy` is not used then; tier: where that store
    keeps its frames ('device', or 'host': pinned host memory).  Frames are named
    frame_%05d.jpg or, as in the reference's Charades loader (charades.py:47), <video id>-%06d.jpg."""
    if resident not in ('decoded', 'compressed'):
        raise ValueError("resident must be 'decoded' or 'compressed' (got %r)" % (resident,))
    if resident == 'compressed':
        from x3dhip.jpegstore import FrameStore
        store = FrameStore(device, threads=threads, tier=tier, **({} if chunk_bytes is None else dict(chunk_bytes=chunk_bytes)))
    else:
        from x3dhip.jpegops import JpegDecoder
        dec = JpegDecoder(device, threads=threads, entropy=entropy)
    videos = {}
    for vid in anno:
        path = os.path.join(root, vid)
        if not os.path.isdir(path):
            continue
        name = FRAME_NAME if os.path.exists(os.path.join(path, FRAME_NAME.format(1))) else vid + '-{:06d}.jpg'
        if resident == 'compressed':
            folder = FrameFolder(path, name)
            ids = None
            for s in range(0, folder.n_frames, 256):
                r = store.add(folder.read(range(s, min(folder.n_frames, s + 256))))
                ids = r if ids is None else range(ids.start, r.stop)
            videos[vid] = StoredVideo(store, ids)
        else:
            videos[vid] = decode_folder(path, device, decoder=dec, name=name)
    return videos
