"""Worker of the grid case of tests/test_gpu_schur_pair_map.py: gridrun_pair's,
with that file's families registered first."""
import gridrun_pair


def _worker(*args):
    import test_gpu_schur_pair_map  # noqa: F401  (adds its families to test_gpu_schur_pair.FAMILIES)
    gridrun_pair._worker(*args)
