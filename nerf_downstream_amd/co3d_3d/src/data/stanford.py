"""S3DIS (Stanford large-scale 3D indoor spaces) point clouds: `ScannetDataset` with other constants, as in the reference
(co3d_3d/src/data/stanford.py:62-112; configs/stanford_semseg.gin).  `<data_root>/stanford_{train,val,test}.txt` list the
PLY files; everything else -- the sample, the down-sampling with label voting, the colour and the geometric program on the
GPU (`prepare_point_batch`) -- is the parent's.  Raw ids 0..13; id 10 is not evaluated, so 0..9 -> 0..9, 10 -> ignore,
11, 12, 13 -> 10, 11, 12."""
from nerf_downstream_amd import gin_lite as gin

from .scannet import ScannetDataset

CLASS_LABELS = ("clutter", "beam", "board", "bookcase", "ceiling", "chair", "column", "door", "floor", "sofa", "table", "wall",
                "window")
VALID_CLASS_IDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13)


@gin.configurable
class StanfordDataset(ScannetDataset):
    NUM_LABELS = 14
    IGNORE_LABELS = tuple(set(range(NUM_LABELS)) - set(VALID_CLASS_IDS))
    DATA_PATH_FILE = {"train": "stanford_train.txt", "val": "stanford_val.txt", "test": "stanford_test.txt"}
    CLASS_LABELS = CLASS_LABELS
    VALID_CLASS_IDS = VALID_CLASS_IDS

    def __init__(self, phase, data_root="datasets/stanford", downsample_voxel_size=0.015, voxel_size=0.03,
                 train_transformations=("ChromaticTranslation", "ChromaticJitter", "CoordinateDropout", "RandomHorizontalFlip",
                                        "RandomRotation", "NormalizeColor"),
                 eval_transformations=("NormalizeColor",), ignore_label=-100, features=("colors",)):
        ScannetDataset.__init__(self, phase, data_root, downsample_voxel_size, voxel_size, train_transformations,
                                eval_transformations, ignore_label, features)
