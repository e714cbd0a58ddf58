"""Data of the 2-D baseline (counterpart of the reference's co3d_2d/src/data/loader.py:232-274): batches
{"images": float [B,3,224,224], "labels": int64 [B]}.  The reference reads rendered PeRFception / CO3D frames from
disk; there is no dataset here, so `SyntheticRenders` draws deterministic 224^2 "renders" -- a class-dependent blob on
a textured background, normalised like ImageNet inputs -- with the same sample dict.

`DataModule(source="files")` reads frames instead (loader.py:73-227 of the reference): `Co3DTrainDataset`, `Co3DEvalDataset` and
their PeRFCeption twins keep the reference's classes, file lists ("<class> <scene> <frames>" per line) and directory layout.  A
worker only decodes the frame to uint8 and draws the recipe (transforms.py, augmix.py); `collate_images` packs the batch and the
trainer hands it to `minkowski.utils.prepare_image_batch`, which runs AugMix and the recipe on the GPU (csrc/image.hip).  With
`PeRFCeptionCo3DTrainDataset.bkgd_on_device` a pasting sample also carries its render and mask, and the same call pastes the render
over the background first (csrc/paste.hip)."""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from nerf_downstream_amd import gin_lite as gin


@gin.configurable
class SyntheticRenders(Dataset):
    def __init__(self, phase="train", num_samples=512, num_classes=51, size=224):
        self.split = 0 if phase == "train" else 1
        self.num_samples = num_samples if self.split == 0 else max(1, num_samples // 4)
        self.num_classes, self.size = num_classes, size

    def __len__(self):
        return self.num_samples

    def __getitem__(self, idx):
        rng = np.random.default_rng(2_000_003 * self.split + idx)
        label = idx % self.num_classes
        crng = np.random.default_rng(4242 + label)
        s = self.size
        yy, xx = np.mgrid[0:s, 0:s].astype(np.float32) / s
        cx, cy, r = 0.3 + 0.4 * crng.random(), 0.3 + 0.4 * crng.random(), 0.12 + 0.2 * crng.random()
        colour = crng.random(3).astype(np.float32)
        blob = np.exp(-(((xx - cx - 0.05 * rng.standard_normal()) ** 2 + (yy - cy - 0.05 * rng.standard_normal()) ** 2) / (2 * r * r)))
        freq = 2 + 6 * crng.random(2)
        tex = 0.5 + 0.5 * np.sin(2 * np.pi * (freq[0] * xx + freq[1] * yy) + rng.random() * 6.28)
        img = colour[:, None, None] * blob[None] + 0.25 * tex[None] + 0.1 * rng.standard_normal((3, s, s)).astype(np.float32)
        img = (img - np.array([0.485, 0.456, 0.406], np.float32)[:, None, None]) / np.array([0.229, 0.224, 0.225], np.float32)[:, None, None]
        return {"images": torch.from_numpy(img.astype(np.float32)), "labels": torch.tensor(label, dtype=torch.int64)}


CLASSES = [
    "apple", "backpack", "ball", "banana", "baseballbat", "baseballglove", "bench", "bicycle", "book", "bottle", "bowl", "broccoli",
    "cake", "car", "carrot", "cellphone", "chair", "couch", "cup", "donut", "frisbee", "hairdryer", "handbag", "hotdog", "hydrant",
    "keyboard", "kite", "laptop", "microwave", "motorcycle", "mouse", "orange", "parkingmeter", "pizza", "plant", "remote", "sandwich",
    "skateboard", "stopsign", "suitcase", "teddybear", "toaster", "toilet", "toybus", "toyplane", "toytrain", "toytruck", "tv",
    "umbrella", "vase", "wineglass",
]
CLASSES_IDX = {k: v for v, k in enumerate(CLASSES)}
TRAIN_RECIPE = ("RandomResizedCrop", "ColorJitter", "RandomHorizontalFlip", "ToTensor", "PCALoss", "Normalize")
EVAL_RECIPE = ("CenterCrop", "ToTensor", "Normalize")


def _read_filelist(filelist_root, phase):
    with open(os.path.join(filelist_root, f"{phase}.txt")) as fp:
        rows = [line.rstrip("/").split() for line in fp if line.strip()]
    for row in rows:
        if len(row) != 3 or row[0] not in CLASSES_IDX:
            raise ValueError(f"{filelist_root}/{phase}.txt: {' '.join(row)!r} is not '<class> <scene> <frames>' of a CO3D class")
    return rows


def _decode(path):
    from PIL import Image  # (imported here: the package imports without Pillow)

    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def _decode_mask(path):
    """Band 0 of a mask file, uint8 [H,W].  A single-band mask is taken as it is (an extension: the reference indexes band 0 of
    an array that then has none); an alpha band is dropped, not multiplied in."""
    from PIL import Image

    with Image.open(path) as im:
        if len(im.getbands()) == 1:
            return np.array(im.convert("L"), dtype=np.uint8)
        return np.ascontiguousarray(np.array(im.convert("RGB"), dtype=np.uint8)[..., 0])


class _Frames(Dataset):
    """What the four datasets share: a frame is decoded to uint8 [H,W,3] and the recipe is drawn, nothing else."""

    def _sample(self, path, label, train):
        return self._sample_of(_decode(path), label, train)

    def _sample_of(self, x, label, train):
        from .transforms import compile_program

        size = (x.shape[1], x.shape[0])
        draws = self.augmix.draw(size, self.transforms.draw) if train else self.transforms.draw(size)
        S = (draws["branches"][0] if train else draws)["S"]
        return {"image": torch.from_numpy(x), "program": torch.from_numpy(compile_program(draws)), "size": S,
                "labels": torch.tensor(label, dtype=torch.int64)}

    def __len__(self):
        return len(self.files)


class _TrainFrames(_Frames):
    subdir, frames_per_scene = "images", None

    def __init__(self, train_transformations, data_root, filelist_root):
        from .transforms import AugMix, Compose

        self.transforms, self.augmix = Compose(train_transformations), AugMix()
        self.files, self.labels, self.num_frames = [], [], []
        for cls_name, scene_name, frame_num in _read_filelist(filelist_root, "train"):
            self.files.append(os.path.join(data_root, cls_name, scene_name, self.subdir))
            self.num_frames.append(int(frame_num) if self.frames_per_scene is None else self.frames_per_scene)
            self.labels.append(CLASSES_IDX[cls_name])

    def __getitem__(self, idx):
        # one frame of the scene, uniformly among its first num_frames entries (the reference indexes os.listdir, whose order the
        # file system chooses; here the names are sorted first)
        random_idx = np.random.randint(self.num_frames[idx])
        fname = sorted(os.listdir(self.files[idx]))[random_idx]
        return self._sample(os.path.join(self.files[idx], fname), self.labels[idx], True)


class _EvalFrames(_Frames):
    subdir = "images"

    def __init__(self, phase, eval_transformations, data_root, filelist_root):
        from .transforms import Compose

        self.transforms = Compose(eval_transformations)
        self.files, self.labels = [], []
        for cls_name, scene_name, _ in _read_filelist(filelist_root, phase):
            images_path = os.path.join(data_root, cls_name, scene_name, self.subdir)
            for frame_name in sorted(os.listdir(images_path)):
                self.files.append(os.path.join(images_path, frame_name))
                self.labels.append(CLASSES_IDX[cls_name])

    def __getitem__(self, idx):
        return self._sample(self.files[idx], self.labels[idx], False)


@gin.configurable
class Co3DTrainDataset(_TrainFrames):
    def __init__(self, train_transformations=TRAIN_RECIPE, data_root="co3d_2d/data/co3d", filelist_root="filelist"):
        super().__init__(train_transformations, data_root, filelist_root)


@gin.configurable
class Co3DEvalDataset(_EvalFrames):
    def __init__(self, phase, eval_transformations=EVAL_RECIPE, data_root="co3d_2d/data/co3d", filelist_root="filelist"):
        super().__init__(phase, eval_transformations, data_root, filelist_root)


@gin.configurable
class PeRFCeptionCo3DTrainDataset(_TrainFrames):
    """`bkgd_aug` is the share of samples whose render is pasted over another scene's background (the reference's loader.py:172-193).
    The paste runs on the GPU only and changes what a sample and a batch hold, so it is opt-in: `bkgd_on_device=True`.  A scene is
    <data_root>/<class>/<scene>/ with the renders in fgbg/, the backgrounds in bg/image000.jpg ... and the masks in
    mask/mask<what follows "image" in the render's name>.  With the binding the draws are the reference's, in its order: the frame,
    p, and only for p < bkgd_aug the background scene and its frame; then BackgroundAug's scale, then AugMix for a frame of the
    background's size.  Without it nothing is drawn but the frame, as before."""
    subdir, frames_per_scene = "fgbg", 50
    bkgd_frames = 50  # frames of a scene's bg/ directory the background is drawn among

    def __init__(self, train_transformations=TRAIN_RECIPE, bkgd_aug=0.0, data_root="co3d_2d/data/perfception", filelist_root="filelist",
                 bkgd_on_device=False):
        if bkgd_aug > 0 and not bkgd_on_device:
            raise NotImplementedError("bkgd_aug > 0: BackgroundAug (pasting the frame over another scene's background) runs on the GPU "
                                      "only and adds the frame and its mask to every pasting sample: bind "
                                      "PeRFCeptionCo3DTrainDataset.bkgd_on_device = True (configs/perfception_bkgd.gin)")
        super().__init__(train_transformations, data_root, filelist_root)
        self.bkgd_aug, self.bkgd_on_device = float(bkgd_aug), bool(bkgd_on_device)
        if self.bkgd_on_device:
            from .transforms import BackgroundAug

            self.bkgd_aug_fun = BackgroundAug()

    def __getitem__(self, idx):
        if not self.bkgd_on_device:
            return super().__getitem__(idx)
        random_idx = np.random.randint(self.num_frames[idx])
        p = np.random.random()
        fname = sorted(os.listdir(self.files[idx]))[random_idx]
        fg = _decode(os.path.join(self.files[idx], fname))
        if not p < self.bkgd_aug:
            return self._sample_of(fg, self.labels[idx], True)
        bkgd_idx = np.random.randint(len(self.files))
        bkgd_frame_idx = np.random.randint(self.bkgd_frames)
        # (the reference finds both directories by replacing "fgbg" anywhere in the path; here they are the scene's own)
        bg = _decode(os.path.join(os.path.dirname(self.files[bkgd_idx]), "bg", f"image{bkgd_frame_idx:03d}.jpg"))
        mask = _decode_mask(os.path.join(os.path.dirname(self.files[idx]), "mask", f"mask{fname[5:]}"))
        rw, rh = self.bkgd_aug_fun.draw((fg.shape[1], fg.shape[0]))
        sample = self._sample_of(bg, self.labels[idx], True)
        sample["paste"] = {"fg": torch.from_numpy(fg), "mask": torch.from_numpy(mask), "size": (rw, rh)}
        return sample


@gin.configurable
class PeRFCeptionCo3DEvalDataset(_EvalFrames):
    subdir = "fgbg"

    def __init__(self, phase, eval_transformations=EVAL_RECIPE, data_root="co3d_2d/data/perfception", filelist_root="filelist"):
        super().__init__(phase, eval_transformations, data_root, filelist_root)


def collate_images(samples):
    """Frames of any sizes -> one batch for `prepare_image_batch`: packed uint8 [sum 3wh] (HWC, one image after the other), offsets
    int64 [B+1] in bytes, sizes int32 [B,2] = (w, h), programs float64 [B, MINK_IMG_PARAMS], size (the S of the recipe), labels.
    Only when a sample of the batch pastes (it has "paste": its "image" is then the background) the batch also holds paste_fg
    uint8 [sum 3wh of the pasted frames], paste_mask uint8 [sum wh of their masks] and paste_table int64 [B, MINK_PASTE_PARAMS]."""
    sizes = {int(s["size"]) for s in samples}
    if len(sizes) != 1:
        raise ValueError(f"one output size per batch, got {sorted(sizes)}")
    images = [s["image"] for s in samples]
    nbytes = [im.numel() for im in images]
    batch = {"packed": torch.cat([im.reshape(-1) for im in images]),
             "offsets": torch.tensor(np.concatenate([[0], np.cumsum(nbytes)]), dtype=torch.int64),
             "sizes": torch.tensor([[im.shape[1], im.shape[0]] for im in images], dtype=torch.int32),
             "programs": torch.stack([s["program"] for s in samples]), "size": torch.tensor(sizes.pop()),
             "labels": torch.stack([s["labels"] for s in samples])}
    if any("paste" in s for s in samples):
        from nerf_downstream_amd._lib import constants

        P = constants("MINK_PASTE_")
        table = torch.zeros(len(samples), P["PARAMS"], dtype=torch.int64)
        fgs, masks, fo, mo = [], [], 0, 0
        for b, s in enumerate(samples):
            if "paste" not in s:
                continue
            fg, mask, (rw, rh) = s["paste"]["fg"], s["paste"]["mask"], s["paste"]["size"]
            for k, v in (("FG_OFFSET", fo), ("MASK_OFFSET", mo), ("FG_W", fg.shape[1]), ("FG_H", fg.shape[0]), ("MASK_W", mask.shape[1]),
                         ("MASK_H", mask.shape[0]), ("RW", rw), ("RH", rh)):
                table[b, P[k]] = int(v)
            fgs.append(fg.reshape(-1)), masks.append(mask.reshape(-1))
            fo, mo = fo + fg.numel(), mo + mask.numel()
        batch["paste_fg"], batch["paste_mask"], batch["paste_table"] = torch.cat(fgs), torch.cat(masks), table
    return batch


def images_to_device(batch, device):
    """A batch of either source on `device` as {"images": float32 [B,3,S,S], "labels"}: a `collate_images` batch (it has
    "programs") goes through the GPU preparation after the copy, any other batch is moved as it is."""
    if "programs" not in batch:
        return {k: v.to(device, non_blocking=True) for k, v in batch.items()}
    from nerf_downstream_amd.minkowski.utils import prepare_image_batch

    with torch.cuda.device(device):
        paste = None
        if "paste_table" in batch:
            paste = {"fg": batch["paste_fg"].to(device, non_blocking=True), "mask": batch["paste_mask"].to(device, non_blocking=True),
                     "table": batch["paste_table"]}
        images = prepare_image_batch(batch["packed"].to(device, non_blocking=True), batch["offsets"], batch["sizes"], batch["programs"],
                                     size=int(batch["size"]), paste=paste)
    return {"images": images, "labels": batch["labels"].to(device, non_blocking=True)}


def _seed_worker(worker_id):
    np.random.seed(torch.initial_seed() % 2**32)  # (the draws use numpy's generator, as the reference's do)


@gin.configurable
class DataModule:
    def __init__(self, num_workers=16, batch_size=32, chunks=32, train_co3d=True, eval_co3d=True, num_samples=512, size=224,
                 source="synthetic"):
        if source not in ("synthetic", "files"):
            raise ValueError(f"DataModule.source = {source!r}: 'synthetic' or 'files'")
        self.num_workers, self.batch_size, self.chunks = num_workers, batch_size, chunks
        self.train_co3d, self.eval_co3d, self.num_samples, self.size, self.source = train_co3d, eval_co3d, num_samples, size, source

    def _files_loader(self, phase, batch_size, shuffle):
        if phase == "train":
            ds = Co3DTrainDataset() if self.train_co3d else PeRFCeptionCo3DTrainDataset()
        else:
            ds = Co3DEvalDataset(phase) if self.eval_co3d else PeRFCeptionCo3DEvalDataset(phase)
        return DataLoader(ds, batch_size=batch_size, num_workers=self.num_workers, shuffle=shuffle, collate_fn=collate_images,
                          persistent_workers=self.num_workers > 0, pin_memory=True, worker_init_fn=_seed_worker)

    def _loader(self, phase, batch_size, shuffle):
        if self.source == "files":
            return self._files_loader(phase, batch_size, shuffle)
        ds = SyntheticRenders(phase, num_samples=self.num_samples, size=self.size)
        g = torch.Generator()
        g.manual_seed(0)
        return DataLoader(ds, batch_size=batch_size, num_workers=self.num_workers, shuffle=shuffle, drop_last=shuffle,
                          persistent_workers=self.num_workers > 0, generator=g)

    def train_dataloader(self):
        return self._loader("train", self.batch_size, True)

    def val_dataloader(self):
        return self._loader("val", self.chunks, False)

    def test_dataloader(self):
        return self._loader("test", self.chunks, False)
