"""Image datasets of the image evals that yield decoded uint8 images through a transform
(evals/image_classification_frozen/transforms.py), in the item layout of the reference's ImageFolder-based datasets
(evals/image_classification_frozen/eval.py:404-409): (transform(image), label).

    SyntheticImages   `data.dataset_name: synthetic_images` -- seeded labelled uint8 images of mixed, non-square sizes
    ImageFolder       `data.dataset_name: image_folder` -- <root>/<class>/<file> read with PIL
"""
import os

import numpy as np
import torch

from .data_manager import _class_wave, _label_and_generator

IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')


class SyntheticImages(torch.utils.data.Dataset):
    """Seeded labelled uint8 images: the decoded-image counterpart of SyntheticImageClassification, as SyntheticFramesClassification
    is of the video one.  Item i depends on (seed, i) alone.  Its label is uniform in [0, num_classes); its pixels are the class
    pattern of SyntheticImageClassification (the same plane wave per channel, drawn from (pattern_seed, label), laid over the
    source image in relative coordinates) plus N(0,1) noise, mapped to bytes as 127.5 + 48 * value and clamped.  Source sizes cycle
    through landscape, portrait, nearly square and wide images around `crop_size`, none square, with sides that are no multiples
    of 4."""

    def __init__(self, length, num_classes, crop_size, transform, seed=0, signal=1.0, pattern_seed=0):
        if transform is None:
            raise ValueError("SyntheticImages needs the eval's image transform (make_transforms)")
        self.length, self.num_classes, self.crop, self.transform = length, num_classes, crop_size, transform
        self.seed, self.signal, self.pattern_seed = seed, signal, pattern_seed
        c = crop_size
        self.sizes = ((c * 8 // 7 + 1, c * 3 // 2 + 2), (c * 3 // 2 + 1, c * 9 // 8 + 2), (c + 1, c + 3), (c * 5 // 4 + 2, c * 2 + 1),
                      (c * 3 // 4 + 1, c + 2))

    def __len__(self):
        return self.length

    def source_size(self, i):
        return self.sizes[(self.seed + i) % len(self.sizes)]

    def image_of(self, i):
        """(uint8 [Hs,Ws,3] array, label) of item i, before the transform."""
        label, g = _label_and_generator(self.seed, i, self.num_classes)
        H, W = self.source_size(i)
        pat = _class_wave(self.pattern_seed, label, self.signal, (H, W)).permute(1, 2, 0)
        img = (127.5 + 48.0 * (torch.randn(H, W, 3, generator=g) + pat)).clamp_(0, 255).to(torch.uint8)
        return img.numpy(), label

    def __getitem__(self, i):
        img, label = self.image_of(i)
        return self.transform(img), label


class ImageFolder(torch.utils.data.Dataset):
    """<root>/<class>/<file>: classes are the sorted directory names, samples the image files of each class in sorted order, read with
    PIL.Image.open(...).convert('RGB') -- the item layout of torchvision's ImageFolder, which the reference's datasets extend.  PIL
    is imported when the first image is read."""

    def __init__(self, root, transform=None):
        if not os.path.isdir(root):
            raise FileNotFoundError(f"ImageFolder: {root} is not a directory")
        self.root, self.transform = root, transform
        self.classes = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
        if not self.classes:
            raise FileNotFoundError(f"ImageFolder: no class directories under {root}")
        self.class_to_idx = {c: k for k, c in enumerate(self.classes)}
        self.samples = []
        for c in self.classes:
            for base, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                self.samples += [(os.path.join(base, f), self.class_to_idx[c]) for f in sorted(files)
                                 if f.lower().endswith(IMG_EXTENSIONS)]
        if not self.samples:
            raise FileNotFoundError(f"ImageFolder: no image files ({', '.join(IMG_EXTENSIONS)}) under {root}")

    def __len__(self):
        return len(self.samples)

    @staticmethod
    def load(path):
        """The uint8 [H,W,3] array of an image file."""
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError("data.dataset_name: image_folder reads its files with PIL (Pillow), which is not installed; install "
                              "Pillow or use data.dataset_name: synthetic_images") from e
        with open(path, 'rb') as f:
            return np.array(Image.open(f).convert('RGB'))

    def __getitem__(self, i):
        path, label = self.samples[i]
        img = self.load(path)
        return (img if self.transform is None else self.transform(img)), label
