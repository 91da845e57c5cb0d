"""Mirror of the reference's ``evaluation`` package for the steps that follow the plane-sweep path:
the geometric-consistency filter (``filtering``), the fusion of the filtered depth maps into a point cloud (``fusibile`` for DTU,
``colmap_fusion`` for YFCC), the point-cloud metrics (``metrics``: radius downsampling and bounded Chamfer distances) and the
COLMAP baseline's PatchMatch stereo (``colmap_stereo``), and the depth-map scores of ``depthmap_eval.py`` (``depthmap_eval``: EPE and
the 1 px / 3 px error rates in one pass).  COLMAP's sparse reconstruction is out of scope."""
