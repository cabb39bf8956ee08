"""Drop-in for the reference's `kinetics.py` (the validation dataset, kinetics.py:161-242): the videos of a subset of the
annotation file, every video as `crops` temporal windows of `sample_duration // gamma_tau` frames, centre crop scaled to
`crop_size`.  The clips come from kinetics_multigrid.DeviceVideoKinetics.val_batch, whatever form its videos have
(frames.py): Kinetics(...) lists the subset and reads folders of JPEG frames, decoded on the GPU (frames.FolderKinetics);
Kinetics.from_dataset takes a ready dataset, for one over a frame store in HBM or pinned host memory
(frames.StoredKinetics: no file is opened during a validation pass).

    from kinetics import Kinetics
    val = Kinetics('data/kinetics/frames_val', 'kinetics_val.json', 'labels.txt', 'validate', sample_duration=80,
                   gamma_tau=5, crops=3, device='cuda:0')
    for clips, labels in val.batches(8, rank, world):       # clips [b, 3, 3, 16, 224, 224], labels [b]
        ...

What differs from the reference: there is no DataLoader -- `batches` yields whole batches on the device -- and the order
is the listing's, where the reference's validation loader shuffles (train_x3d_kinetics_multigrid.py:151).  The totals of a
validation phase (videos, correct counts, the sum of the losses) do not depend on the order; the reference's "Cls Loss",
a mean of batch means, does in its last digits when the last batch is short, because which videos share that batch then
changes their weight.
"""
from frames import FolderKinetics


class Kinetics:
    """Validation videos of `subset` under root_path (make_dataset, kinetics.py:98-158: folders that are missing or hold
    81 frames or fewer are skipped).  class_labels: the label file (or a list of class names); annotation_path: the
    annotation json (or its dict)."""

    def __init__(self, root_path, annotation_path, class_labels, subset, sample_duration=16, gamma_tau=5, crops=10,
                 crop_size=224, device='cuda:0', threads=8, entropy='host'):
        decode = {} if entropy == 'host' else dict(entropy=entropy)      # 'host' is FolderKinetics' own default
        self._init(FolderKinetics.from_annotation(root_path, annotation_path, class_labels, subset,
                                                  sample_duration=sample_duration, gamma_tau=gamma_tau,
                                                  crop_size=crop_size, device=device, threads=threads, **decode), crops)

    def _init(self, dataset, crops):
        if int(crops) < 2:
            raise ValueError("Kinetics: the window step divides by crops - 1 (kinetics.py:220), so crops >= 2")
        self.dataset, self.crops = dataset, int(crops)
        self.sharded = None
        self.sample_duration, self.gamma_tau = dataset.sample_duration, dataset.gamma_tau
        self.frames = self.sample_duration // self.gamma_tau

    @classmethod
    def from_dataset(cls, dataset, crops=10, sharded=None):
        """Over a ready kinetics_multigrid.DeviceVideoKinetics (frames.FolderKinetics and frames.StoredKinetics construct
        one): anything with __len__ and val_batch(indices, crops=).  sharded=(rank, world): the dataset already holds only
        the videos rank, rank + world, ... of the listing (frames.StoredKinetics.from_pack(..., rank=, world=)); shard() and
        batches() then take that rank and world only, and give all of it."""
        self = cls.__new__(cls)
        self._init(dataset, crops)
        if sharded is not None:
            self.sharded = (int(sharded[0]), int(sharded[1]))
        return self

    def __len__(self):
        return len(self.dataset)

    def shard(self, rank=0, world=1):
        """The videos of one rank: rank, rank + world, ... in listing order."""
        if not 0 <= rank < world:
            raise ValueError("rank %d outside a world of %d" % (rank, world))
        if self.sharded is not None:
            if (rank, world) != self.sharded:
                raise ValueError("this dataset holds the shard of rank %d of %d, not of rank %d of %d" % (self.sharded + (rank, world)))
            return list(range(len(self)))
        return list(range(rank, len(self), world))

    def batches(self, batch_size, rank=0, world=1):
        """Yields (clips float32 [b, crops, 3, T, S, S], labels int64 [b]) on the device over this rank's shard;
        b = batch_size except in a short last batch."""
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        mine = self.shard(rank, world)
        for i in range(0, len(mine), batch_size):
            yield self.dataset.val_batch(mine[i:i + batch_size], crops=self.crops)
