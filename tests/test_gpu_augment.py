"""The geometric training augmentation of data.GPUTransform / NoisyTransform on the GPU: the augmented
transform equals, bit for bit, the plain transform applied to crops transformed by the restatement
(tests/dihedral_ref.py) with ids redrawn from an identically seeded generator; no other draw moves."""
import pytest
import torch

import dihedral_ref as ref
from image_super_resolution_amd import data

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, T, SCALE, SEED = 6, 48, 4, 11


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


@pytest.fixture(scope="module")
def crops():
    return torch.randint(0, 256, (N, 3, T, T), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))


def redraw(augment: str, n: int, seed: int = SEED, calls: int = 1) -> list:
    """The ids of the `calls`-th call of a transform seeded with `seed`, drawn as the docstring says."""
    g = torch.Generator(device=DEV).manual_seed(seed + data.AUGMENT_SEED_OFFSET)
    for _ in range(calls):
        if augment == "flip":
            ids = torch.randint(0, 2, (n,), generator=g, device=DEV) * 4
        else:
            ids = torch.randint(0, 8, (n,), generator=g, device=DEV)
    return ids.tolist()


@pytest.mark.parametrize("augment", ["flip", "dihedral"])
@pytest.mark.parametrize("lr_filter", ["cv2", "bicubic"])
def test_augmented_equals_plain_on_transformed_crops(crops, lr_filter, augment):
    tf = data.GPUTransform(SCALE, device=DEV, lr_filter=lr_filter, seed=SEED, augment=augment)
    plain = data.GPUTransform(SCALE, device=DEV, lr_filter=lr_filter, seed=SEED, augment="none")
    for call in (1, 2):  # the generator moves on from call to call
        ids = redraw(augment, N, calls=call)
        hr, lr = tf(crops)
        want_hr, want_lr = plain(ref.apply_ref(crops, ids))
        assert torch.equal(hr, want_hr) and torch.equal(lr, want_lr), (call, ids)
    assert set(ids) <= ({0, 4} if augment == "flip" else set(range(8)))


def test_the_ids_do_occur():
    assert len(set(redraw("dihedral", N))) >= 3
    assert set(redraw("flip", N)) | set(redraw("flip", N, calls=2)) == {0, 4}


@pytest.mark.parametrize("augment", ["flip", "dihedral"])
def test_degradation_draws_do_not_move(crops, augment):
    def make(aug):
        return data.GPUTransform(SCALE, device=DEV, lr_filter="random", seed=SEED, augment=aug,
                                 degrade=data.LRDegrade.preset("blind", device=DEV, seed=5))
    tf, plain = make(augment), make("none")
    ids = redraw(augment, N)
    moved = ref.apply_ref(crops, ids)
    hr, lr = tf(crops)
    # hr is made from the clean (transformed) crops: what it is without any degradation
    hr_clean, _ = data.GPUTransform(SCALE, device=DEV, lr_filter="random", seed=SEED)(moved)
    assert torch.equal(hr, hr_clean)
    # same filter draw, same degradation draws: the un-augmented transform on the moved crops gives the same lr
    want_hr, want_lr = plain(moved)
    assert torch.equal(hr, want_hr) and torch.equal(lr, want_lr)
    assert torch.equal(tf.degrade.gen.get_state(), plain.degrade.gen.get_state())
    assert torch.equal(tf.degrade.host_gen.get_state(), plain.degrade.host_gen.get_state())
    assert torch.equal(tf.gen.get_state(), plain.gen.get_state())


def test_noisy_transform_flip_on_non_square_crops():
    x = torch.randint(0, 256, (N, 3, 32, 48), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    tf = data.NoisyTransform(device=DEV, seed=SEED, augment="flip")
    plain = data.NoisyTransform(device=DEV, seed=SEED)
    ids = redraw("flip", N)
    assert len(set(ids)) == 2
    moved = ref.apply_ref(x, [0] * N).clone()
    for i, k in enumerate(ids):
        moved[i] = ref.apply_ref(x[i], k)
    clean, noisy = tf(x)
    want_clean, want_noisy = plain(moved)
    assert torch.equal(clean, want_clean)  # the clean target is the flipped crop's
    assert torch.equal(noisy, want_noisy)  # and the noise draws are the ones of the plain transform
    with pytest.raises(ValueError, match="square"):
        data.NoisyTransform(device=DEV, seed=SEED, augment="dihedral")(x)


def test_none_is_the_transform_without_the_argument(crops):
    for kw in (dict(lr_filter="cv2"), dict(lr_filter="random"),
               dict(lr_filter="bicubic", degrade=None)):
        a = data.GPUTransform(SCALE, device=DEV, seed=SEED, augment="none", **kw)(crops)
        b = data.GPUTransform(SCALE, device=DEV, seed=SEED, **kw)(crops)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), kw
    a = data.NoisyTransform(device=DEV, seed=SEED, augment="none")(crops)
    b = data.NoisyTransform(device=DEV, seed=SEED)(crops)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert data.GPUTransform(SCALE, device=DEV, augment="none").augment.gen is None  # nothing drawn, nothing launched


def test_dihedral_needs_square_crops():
    """GPUTransform itself only takes square crops; the augmentation's own refusal is NoisyTransform's to show
    (above).  Here: the primitive behind both."""
    x = torch.zeros(2, 3, 32, 48, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="square"):
        data.GPUTransform(SCALE, device=DEV, seed=SEED, augment="dihedral")(x)
    aug = data._Augment("GPUTransform", "dihedral", SEED, DEV)
    with pytest.raises(ValueError, match="square"):
        aug(x)
    assert tuple(data._Augment("GPUTransform", "flip", SEED, DEV)(x).shape) == tuple(x.shape)
