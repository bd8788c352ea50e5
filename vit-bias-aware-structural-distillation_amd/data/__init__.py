"""Dual-view input pipeline (reference ``src/data/datasets.py``) over local data."""
from .datasets import (create_dataloaders, create_eval_loader, build_eval_transform, dataset_info,  # noqa: F401
                       get_channel_stats, get_subset_indices, is_local_dataset)
from .device_views import (DeviceDualView, DeviceEvalView, augment_records, clean_records, clean_view_geometry,  # noqa: F401
                           draw_augment_params, pack_images)
