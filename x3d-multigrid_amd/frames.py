"""Folders of JPEG frames as a data source: the reference's on-disk protocol (kinetics.py:43-51: `frame_%05d.jpg`, 1-based)
read from disk on the host and decoded on the GPU by libx3djpeg.so, bit-exact with the PIL decode of the reference's loader.

A video reaches a dataset (kinetics_multigrid.DeviceVideoKinetics, charades.Charades) in one of two forms.  Decoded: a uint8
tensor [n, H, W, 3] in HBM (decode_folder).  Lazy: an object with .shape = (n_frames, H, W, 3), .device, .source -- something
with decode_into(requests, dst), a JpegDecoder or a FrameStore -- and .requests(idx), what that source takes for the
0-based frames idx (ValueError for a frame it cannot serve):

FolderVideo      a FrameFolder and the JpegDecoder that decodes it; the requests are the files' bytes
StoredVideo      frames of a x3dhip.jpegstore.FrameStore (prepared scans, about the size of the files, in HBM or in pinned
                 host memory); the requests are frame ids.  WindowedVideo: one of which only some frames are stored

gather_frames (x3dhip.clip_input, also reachable from here) is the one place where lazy videos are decoded: per batch, exactly the frames the batch draws, one
decode_into per source and frame size.  The datasets call it on their samples and hand the result to the clip kernels, so
a dataset may mix all three kinds of video.  A new way of keeping frames resident is a new lazy video, not a new dataset.

FrameFolder      one video on disk: frame count and size from the listing and the first file's header, raw bytes on demand
FolderKinetics   DeviceVideoKinetics constructed over folders (FolderVideos on one decoder)
StoredKinetics   DeviceVideoKinetics constructed over a store: filled from folders (from_annotation) or read from a pack
                 file (from_pack; FrameStore.save / load, tools/pack_frames.py writes one without a GPU)
charades_videos  the `videos` dict of charades.Charades from folders, decoded or as StoredVideos
"""
import json
import os

import torch

from kinetics_multigrid import DeviceVideoKinetics
from x3dhip.clip_input import gather_frames, is_lazy  # noqa: F401  (the protocol's two functions, beside the clip kernels' host side)

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


class LazyVideo:
    """What the lazy videos share: .frames(idx) decodes the 0-based frames idx now, uint8 [len(idx), H, W, 3] on .device."""

    def frames(self, idx):
        requests = self.requests(list(idx))
        out = torch.empty((len(requests),) + self.shape[1:], dtype=torch.uint8, device=self.device)
        return self.source.decode_into(requests, out)


class FolderVideo(LazyVideo):
    """A FrameFolder decoded by `decoder` (a JpegDecoder): the requests are the bytes of the files."""

    def __init__(self, folder, decoder):
        self.folder, self.source, self.device = folder, decoder, decoder.device
        self.shape = (folder.n_frames, folder.height, folder.width, 3)
        self.requests = folder.read


class FolderKinetics(DeviceVideoKinetics):
    """DeviceVideoKinetics over frame folders (paths or FrameFolders), all read through one JpegDecoder (.decoder): per
    batch only the drawn frames are read and decoded."""

    def __init__(self, folders, labels, *args, device='cuda:0', threads=8, entropy='host', **kw):
        from x3dhip.jpegops import JpegDecoder
        if len(folders) != len(labels) or not folders:
            raise ValueError("one label per folder, at least one folder")
        self.folders = [f if isinstance(f, FrameFolder) else FrameFolder(f) for f in folders]
        self.decoder = JpegDecoder(device, threads=threads, entropy=entropy)
        super().__init__([FolderVideo(f, self.decoder) for f in self.folders], labels, *args, **kw)

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


class StoredVideo(LazyVideo):
    """One video in a FrameStore: frames ids[0], ids[1], ... of the store, all of one size.  .shape is what the decoded
    video's would be; the requests are the store's frame ids."""

    def __init__(self, store, ids):
        ids = range(ids.start, ids.stop) if isinstance(ids, range) and ids.step == 1 else ids
        if not isinstance(ids, range) or len(ids) < 1 or ids.start < 0 or ids.stop > len(store):
            raise ValueError("ids must be a non-empty range of frame ids of the store")
        w, h = store.width[ids.start:ids.stop], store.height[ids.start:ids.stop]
        if (w != w[0]).any() or (h != h[0]).any():
            raise ValueError("the frames of a video are of one size")
        self.store = self.source = store
        self.ids, self.device = ids, store.device
        self.shape = (len(ids), int(h[0]), int(w[0]), 3)

    def requests(self, idx):
        """The store's ids of the 0-based frames idx."""
        n = self.shape[0]
        for i in idx:
            if not 0 <= i < n:
                raise ValueError("frame %d outside the %d frames of the video" % (i, n))
        return [self.ids.start + i for i in idx]


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

    def requests(self, idx):
        try:
            return [self.ids.start + self._at[int(i)] for i in idx]
        except KeyError as e:
            raise ValueError("frame %s of video %s is not in the pack (it holds %d of its %d frames)" % (
                e.args[0], self.name, len(self.ids), self.shape[0])) from None


def val_window_frames(n_frames, gamma_tau, sample_duration, crops):
    """The sorted 0-based frames of a video that the validation windows of kinetics.Kinetics draw (they do not depend on
    anything but these four numbers)."""
    from x3dhip.clip_input import val_crop_indices
    return sorted({int(i) for idx in val_crop_indices(n_frames, gamma_tau, sample_duration, crops) for i in idx})


def add_folder(store, folder, want=None, chunk=256):
    """Adds the 0-based frames `want` (None: all of them) of a FrameFolder to the store, `chunk` files at a time.  Returns
    the range of their ids."""
    want = range(folder.n_frames) if want is None else want
    first = len(store)
    for s in range(0, len(want), chunk):
        store.add(folder.read(want[s:s + chunk]))
    return range(first, len(store))


def fill_store(store, entries, windows=None, chunk=256):
    """Adds the frames of entries ([(FrameFolder, label)]) to the store; windows: dict(gamma_tau=, sample_duration=,
    crops=) to store only the frames the validation windows draw.  Returns the pack meta of the videos: name (the folder
    relative to nothing: its path's last two parts), label, first id, stored frames, n_frames and index (the original
    frame index of every stored frame; None stands for all of them in order)."""
    videos = []
    for folder, label in entries:
        index = None if windows is None else val_window_frames(folder.n_frames, **windows)
        ids = add_folder(store, folder, index, chunk)
        videos.append(dict(name="/".join(os.path.normpath(folder.path).split(os.sep)[-2:]), label=int(label),
                           first=ids.start, frames=len(ids), n_frames=folder.n_frames, index=index))
    return dict(videos=videos, windows=windows)


class StoredKinetics(DeviceVideoKinetics):
    """DeviceVideoKinetics over the StoredVideos of one FrameStore (.store); meta: the pack meta they came with.  With
    equal rng seeds a batch is bit for bit the FolderKinetics batch of the same videos."""

    def __init__(self, videos, labels, *args, meta=None, **kw):
        if len(videos) != len(labels) or not videos:
            raise ValueError("one label per video, at least one video")
        super().__init__(list(videos), list(labels), *args, **kw)
        self.store, self.meta = self.videos[0].store, meta

    @classmethod
    def from_annotation(cls, root, anno_json, labels_txt, subset, tier='device', device='cuda:0', threads=8,
                        chunk_bytes=None, rank=0, world=1, index_bits=None, **kw):
        """The listing of FolderKinetics.from_annotation, its videos i % world == rank read into a FrameStore of `tier`
        (index_bits: with a sync index of that granularity; None: without)."""
        from x3dhip.jpegstore import FrameStore
        entries = list_annotation(root, anno_json, labels_txt, subset)[rank::world]
        if not entries:
            raise ValueError("rank %d of %d has no video of subset %r under %s" % (rank, world, subset, root))
        store = FrameStore(device, threads=threads, tier=tier, chunk_bytes=chunk_bytes, index_bits=index_bits)
        meta = fill_store(store, entries)
        return cls._over(store, meta, [range(v["first"], v["first"] + v["frames"]) for v in meta["videos"]], **kw)

    @classmethod
    def from_pack(cls, path, device='cuda:0', tier='device', rank=0, world=1, chunk_bytes=None, index_bits=None, **kw):
        """The videos i % world == rank of a pack file (tools/pack_frames.py, or FrameStore.save with fill_store's meta):
        only their frames are read.  index_bits: None uses the pack's sync index if it has one beside it (path + '.idx');
        an int builds an index of that granularity while loading."""
        from x3dhip.jpegstore import FrameStore
        meta = FrameStore.read_meta(path)
        if not isinstance(meta, dict) or not isinstance(meta.get("videos"), list):
            raise ValueError("%s carries no list of videos" % path)
        mine = meta["videos"][rank::world]
        if not mine:
            raise ValueError("rank %d of %d has no video of %s" % (rank, world, path))
        store, _, id_map = FrameStore.load(path, device, tier=tier, chunk_bytes=chunk_bytes, index=index_bits,
                                           ranges=[range(v["first"], v["first"] + v["frames"]) for v in mine])
        return cls._over(store, dict(meta, videos=mine), id_map, **kw)

    @classmethod
    def _over(cls, store, meta, ids, **kw):
        videos = [StoredVideo(store, r) if v.get("index") is None else
                  WindowedVideo(store, r, v["n_frames"], v["index"], v["name"]) for v, r in zip(meta["videos"], ids)]
        return cls(videos, [v["label"] for v in meta["videos"]], meta=meta, **kw)


def charades_videos(root, anno, device, threads=8, entropy='host', resident='decoded', chunk_bytes=None, tier='device',
                    index_bits=None):
    """{video id: video} for every video of the annotation dict that has a folder under root: the `videos` argument of
    charades.Charades and the Charades training scripts.  resident='decoded': uint8 [n, H, W, 3], decoded whole.
    resident='compressed': StoredVideo over one FrameStore shared by all videos (chunk_bytes: its arena chunk size),
    decoded batch by batch on the GPU, Huffman decoding included; `entropy` is not used then; tier: where that store
    keeps its frames ('device', or 'host': pinned host memory); index_bits: that store keeps a sync index of that
    granularity and decodes through it.  Frames are named
    frame_%05d.jpg or, as in the reference's Charades loader (charades.py:47), <video id>-%06d.jpg."""
    if resident not in ('decoded', 'compressed'):
        raise ValueError("resident must be 'decoded' or 'compressed' (got %r)" % (resident,))
    if resident == 'compressed':
        from x3dhip.jpegstore import FrameStore
        store = FrameStore(device, threads=threads, tier=tier, chunk_bytes=chunk_bytes, index_bits=index_bits)
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
            videos[vid] = StoredVideo(store, add_folder(store, FrameFolder(path, name)))
        else:
            videos[vid] = decode_folder(path, device, decoder=dec, name=name)
    return videos
