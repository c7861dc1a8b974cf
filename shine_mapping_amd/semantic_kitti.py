"""The label definition of a SemanticKITTI-style drive: which class a raw 16-bit label id stands for, and the colour of a class.

    label_map = LabelMap.from_config(config)
    label_map.lut       int32 [65536]: raw id -> class, -1 for an id the map does not know (shine_sem_frame_filter reads it)
    label_map.colors    fp64 [n_class, 3] in 0..1, or None
    label_map.n_class   config.sem_class_count + 1 (the classes are 0 .. sem_class_count, 0 = unlabeled)

No table is kept here: the map comes from the config (dicts or a yaml file in the layout of SemanticKITTI's own semantic-kitti.yaml)
or, at run time, from the reference's utils.semantic_kitti_utils when that module can be imported — the mechanism
mesher._sem_color_map uses for the mesh colours.
"""
from __future__ import annotations

import numpy as np

N_RAW = 1 << 16  # the lower 16 bits of a .label word are the semantic id, the upper 16 the instance


class LabelMap:
    def __init__(self, learning_map, color_map=None, sem_class_count=20):
        """learning_map: {raw id: class}; color_map: {class: (r, g, b) 0-255} or None"""
        n_class = int(sem_class_count) + 1
        lut = np.full(N_RAW, -1, dtype=np.int32)
        for raw, cls in dict(learning_map).items():
            raw, cls = int(raw), int(cls)
            if not 0 <= raw < N_RAW:
                raise ValueError("LabelMap: raw label id %d is not a 16-bit id" % raw)
            if not 0 <= cls <= int(sem_class_count):
                raise ValueError("LabelMap: raw id %d maps to class %d, outside [0, sem_class_count = %d]"
                                 % (raw, cls, int(sem_class_count)))
            lut[raw] = cls
        colors = None
        if color_map:
            colors = np.zeros((n_class, 3), dtype=np.float64)
            for cls, rgb in dict(color_map).items():
                cls = int(cls)
                if not 0 <= cls <= int(sem_class_count):
                    raise ValueError("LabelMap: the colour map names class %d, outside [0, sem_class_count = %d]"
                                     % (cls, int(sem_class_count)))
                colors[cls] = np.asarray(rgb, dtype=np.float64).reshape(3) / 255.0
        self.lut, self.colors, self.n_class = lut, colors, n_class
        self._device = {}

    @classmethod
    def from_yaml(cls, path, sem_class_count=20):
        """semantic-kitti.yaml's layout: learning_map (raw id -> class); colours from color_map (BGR, keyed by RAW id) through
        learning_map_inv (class -> the raw id that represents it)"""
        import yaml

        with open(path) as fh:
            doc = yaml.safe_load(fh)
        if not isinstance(doc, dict) or "learning_map" not in doc:
            raise ValueError("LabelMap: %s holds no learning_map" % path)
        color_map = None
        if "color_map" in doc and "learning_map_inv" in doc:
            color_map = {}
            for c, raw in doc["learning_map_inv"].items():
                if raw in doc["color_map"]:
                    b, g, r = doc["color_map"][raw]
                    color_map[int(c)] = (r, g, b)
        return cls(doc["learning_map"], color_map, sem_class_count)

    @classmethod
    def from_config(cls, config):
        count = int(getattr(config, "sem_class_count", 20))
        learning = getattr(config, "sem_label_map", None)
        if learning:
            return cls(learning, getattr(config, "sem_color_map", None), count)
        path = getattr(config, "label_map_path", None)
        if path:
            return cls.from_yaml(path, count)
        try:
            from utils.semantic_kitti_utils import sem_kitti_color_map, sem_kitti_learning_map
        except Exception:
            raise ValueError("LabelMap.from_config: no label definition — set config.sem_label_map (dict raw id -> class), or "
                             "config.label_map_path (a yaml in semantic-kitti.yaml's layout), or make the reference's "
                             "utils.semantic_kitti_utils importable") from None
        return cls(sem_kitti_learning_map, sem_kitti_color_map, count)

    def device_lut(self, device):
        """the look-up table on `device` (uploaded once per device)"""
        import torch

        key = str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.lut).to(device)
        return self._device[key]

    def device_colors(self, device):
        import torch

        key = "c" + str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.colors).to(device)
        return self._device[key]
