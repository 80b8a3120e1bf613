"""A seeded slice of the randomised soak (profiles/soak_raster.py runs the same generator for minutes) inside the GPU
suite: ~200 random frames through the mode product of the operator -- binning structure x forward blend kernel x per-tile
schedule x gradient-tensor route (fresh / kept rows / kept full, with / without torch's use count) x accumulator kept or cleared -- against
the C oracle with the parity tests' checks."""
import pytest

import soak_cases

pytestmark = pytest.mark.gpu

CASES = 200


def test_seeded_slice_of_the_soak(oracle, gpu):
    rec = soak_cases.run(gpu, oracle, seed=20251005, cases=CASES)
    assert rec["cases"] == CASES
    assert rec["modes_met"] >= 60, rec["by_mode"]                         # of 2 x 2 x 4 x 3 x 2 x 2 = 192 combinations
    # pixels on the 1/255 or T = 1e-4 edge happen; frames beyond the tests' own count band must stay the exception
    assert rec["cases_beyond_the_tests_pixel_count_band"] <= CASES // 20, rec


CAMERA_CASES = 100


def test_seeded_slice_of_the_soak_through_sensor_cameras(oracle, gpu):
    """The same generator, another seed, every frame through the camera its case names: the centred one or one of
    helpers.CAMERAS (principal point off the centre, fx != fy, tele / wide, the ToF camera's default planes)."""
    import helpers as Hh
    rec = soak_cases.run(gpu, oracle, seed=20261016, cases=CAMERA_CASES, cameras=True)
    print("soak through sensor cameras: %.1f s, %s, deepest tile list %d" % (rec["seconds"], rec["by_camera"], rec["deepest_tile_list"]))
    assert rec["cases"] == CAMERA_CASES
    assert set(rec["by_camera"]) == {str(c) for c in [None] + list(Hh.CAMERAS)}, rec["by_camera"]
    assert rec["cases_beyond_the_tests_pixel_count_band"] <= CAMERA_CASES // 20, rec
