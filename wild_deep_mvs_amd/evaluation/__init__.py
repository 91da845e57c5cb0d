"""Mirror of the reference's ``evaluation`` package for the steps that follow the plane-sweep path:
the geometric-consistency filter (``filtering``) and the fusion of the filtered depth maps into a point cloud (``fusibile``).
The rest of the reference's evaluation pipeline (COLMAP glue, metrics) is out of scope and keeps calling it."""
