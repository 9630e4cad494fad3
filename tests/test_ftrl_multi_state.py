"""CPU: the multi-model image file (ftrl.save_multi_state / load_multi_state)
and its separation from the single-model one."""
import numpy as np
import pytest

from parameter_server_amd import ftrl


def image(n=5, m=3):
    rng = np.random.default_rng(3)
    w = rng.standard_normal((n, m))
    w[:1, 0] = -0.0
    return (np.arange(n, dtype=np.uint64) * 7, rng.integers(0, 1 << 40, size=n, dtype=np.uint64),
            rng.integers(0, 9, size=n, dtype=np.uint64), w, rng.standard_normal((n, m)))


PARAMS = [dict(alpha=0.1 * (j + 1), beta=1.0, lambda1=0.5 * j, lambda2=0.1) for j in range(3)]


@pytest.mark.parametrize("n", (0, 5))
def test_round_trip(tmp_path, n):
    path = str(tmp_path / "sweep.ckpt")
    img = image(n)
    ftrl.save_multi_state(path, *img, PARAMS, frozen=True, objv=np.arange(3.0))
    st = ftrl.load_multi_state(path)
    for name, a in zip(("keys", "pos", "neg", "w", "z"), img):
        assert st[name].shape == a.shape and st[name].tobytes() == a.tobytes(), name
    for name in ("alpha", "beta", "lambda1", "lambda2"):
        assert st[name].tolist() == [p[name] for p in PARAMS]
    assert (int(st["m"]), int(st["frozen"])) == (3, 1) and st["objv"].tolist() == [0.0, 1.0, 2.0]
    with pytest.raises(ValueError):
        ftrl.save_multi_state(path, *img, PARAMS, m=4)  # a field of the format
    with pytest.raises(ValueError):
        ftrl.save_multi_state(path, *img[:3], img[3][:, :2], img[4], PARAMS)  # w is not [n, m]


def test_each_loader_rejects_the_other_image_and_an_unknown_version(tmp_path):
    multi, scalar, future = (str(tmp_path / name) for name in ("multi", "scalar", "future"))
    img = image()
    ftrl.save_multi_state(multi, *img, PARAMS)
    ftrl.save_state(scalar, *img[:3], img[3][:, 0], img[4][:, 0], 0.1, 1.0, 0.0, 0.1)
    with pytest.raises(ValueError, match="multi-model"):
        ftrl.load_state(multi)
    with pytest.raises(ValueError, match="single-model"):
        ftrl.load_multi_state(scalar)
    assert ftrl.load_state(scalar)["w"].tobytes() == np.ascontiguousarray(img[3][:, 0]).tobytes()
    with np.load(multi) as f:
        fields = {name: f[name] for name in f.files}
    fields[ftrl.MULTI_VERSION_FIELD] = np.array(ftrl.MULTI_STATE_VERSION + 1, np.int64)
    with open(future, "wb") as f:
        np.savez(f, **fields)
    with pytest.raises(ValueError, match="version"):
        ftrl.load_multi_state(future)
