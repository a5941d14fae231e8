"""MSK-INPAINT v1 beside cv2.inpaint(image, mask, 5, INPAINT_TELEA), wherever cv2 is installed (it skips elsewhere).  The two march
in different orders -- cv2 by its heap, the spec level by level -- so inside the mask only the mean absolute difference is reported;
outside the mask both must leave every pixel as it was."""
import numpy as np
import pytest

import maskinpaint_np as ref

cv2 = pytest.importorskip("cv2")


@pytest.mark.parametrize("name", ["photograph", "ramp"])
def test_outside_the_mask_nothing_differs_and_the_inside_is_reported(name):
    F = ref.fixture_mask()
    H, W = F.shape
    img = ref.photograph(H, W, 5) if name == "photograph" else ref.ramp(H, W, 2, 3, 7)
    ours, _K = ref.inpaint(img, F)
    theirs = cv2.inpaint(img, np.where(F, 255, 0).astype(np.uint8), 5, cv2.INPAINT_TELEA)
    assert np.array_equal(ours[~F], theirs[~F]) and np.array_equal(ours[~F], img[~F])
    diff = np.abs(ours[F].astype(np.int32) - theirs[F].astype(np.int32))
    print(f"{name}: mean absolute difference inside the mask {diff.mean():.3f}, largest {int(diff.max())}")
