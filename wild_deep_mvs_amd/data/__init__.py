"""Per-view input preparation of the reference's datasets (``data/MVSDataset.py``, ``data/md_yao.py``) as functions on device
tensors; no ``Dataset`` classes."""
