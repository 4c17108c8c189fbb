"""CPU tests of per-image inpainting masks: the mask bank's tables against the single-mask operators (the engine's and
oracle/operators.py::Inpainting), which sampler call restores which image -- and so which mask, i % N -- in every sharding
and fusing mode of the runner, the rejected inputs, and the argument checks of the four `*_pi_*` entry points (made
before any launch, so they run without a GPU)."""
import ctypes
import types

import numpy as np
import pytest
import torch

D = 32
PI_SYMBOLS = ["ddnm_op_inpaint_A_pi_f32", "ddnm_op_inpaint_pinv_pi_f32", "ddnm_step_inpaint_pi_f32",
              "ddnm_step_inpaint_pi_keyed_f32"]


def bank_masks(d):
    """The deterministic bank [3, d, d] (1 = kept): M0 keeps p % 3 != 0, M1 the first five pixels, M2 all but the 15 x 15
    square of rows and columns 8..22.  At d = 32: 682 / 5 / 799 kept pixels, rows of 2046 / 15 / 2397 entries -- three
    lengths, none a multiple of 4, all shorter than y_dim = 2400."""
    p = np.arange(d * d)
    m0 = (p % 3 != 0).astype(np.float32)
    m1 = (p < 5).astype(np.float32)
    m2 = np.ones((d, d), dtype=np.float32)
    m2[8:23, 8:23] = 0
    return np.stack([m0.reshape(d, d), m1.reshape(d, d), m2])


def single_mask_operator(mask2d, d, device):
    """The engine's existing one-mask Inpainting, built as build_operator builds it."""
    from ddnm_amd.functions import svd_operators as E
    from oracle import operators
    return E.Inpainting(3, d, operators.Inpainting.missing_from_mask(mask2d), device)


def test_bank_tables_match_the_single_mask_operators():
    from ddnm_amd.functions import svd_operators as E
    from oracle import operators
    masks = bank_masks(D)
    bank = E.InpaintingBank(3, D, masks, "cpu")
    assert len(bank) == 3 and bank.n_kept == [682, 5, 799] and bank.y_dim == 2400
    flat = E.InpaintingBank(3, D, masks.reshape(3, -1), "cpu")           # [N, S*S] is the same bank
    for i in range(3):
        one = single_mask_operator(masks[i], D, "cpu")
        assert one.n_kept == bank.n_kept[i]
        assert torch.equal(bank.rank[i], one.rank) and torch.equal(flat.rank[i], one.rank)
        assert torch.equal(bank.kept_mask[i], one.kept_mask)
        # rank inverts the oracle's list of kept HWC entries: pixel p is kept entry rank[p] of channel 0
        kept = operators.Inpainting(3, D, operators.Inpainting.missing_from_mask(masks[i])).kept
        pix = torch.nonzero(bank.rank[i] >= 0).reshape(-1)
        assert torch.equal(kept[0::3], pix * 3) and torch.equal(bank.rank[i][pix].long(), torch.arange(len(pix)))


def test_for_images_narrow_and_concat_pick_rows_by_index_mod_n():
    from ddnm_amd.functions import svd_operators as E
    bank = E.InpaintingBank(3, D, bank_masks(D), "cpu")
    op = bank.for_images([2, 0, 1, 5, 3])
    assert len(op) == 5 and op.rows == [2, 0, 1, 2, 0] and op.n_kept == [799, 682, 5, 799, 682] and op.y_dim == 2400
    for b, r in enumerate(op.rows):
        assert torch.equal(op.rank[b], bank.rank[r])
        assert torch.equal(op.kept3[b], bank.kept_mask[r].expand(3, -1))
    part = op.narrow(1, 4)
    assert part.rows == [0, 1, 2] and torch.equal(part.rank, op.rank[1:4]) and part.rank.data_ptr() == op.rank[1].data_ptr()
    both = E.PerImageInpainting.concat([op.narrow(3, 5), part])
    assert both.rows == [2, 0, 0, 1, 2] and torch.equal(both.rank, torch.cat([op.rank[3:5], op.rank[1:4]], 0))
    assert torch.equal(both.kept3, torch.cat([op.kept3[3:5], op.kept3[1:4]], 0))
    for bad in ((0, 0), (2, 6), (-1, 2)):
        with pytest.raises(ValueError):
            op.narrow(*bad)
    with pytest.raises(ValueError):
        bank.for_images([])
    for name in ("singulars", "V", "Vt", "U", "Ut", "add_zeros", "At", "A_pinv_eta"):
        with pytest.raises(NotImplementedError, match="ragged"):
            getattr(op, name)(torch.zeros(5, 3 * D * D))
    # an operator is tied to its batch: another batch size is refused before anything is launched
    x = torch.zeros(4, 3, D, D)
    for call in (lambda: op.A(x), lambda: op.A_pinv(torch.zeros(4, 2400)), lambda: op.Lambda(x, 1.0, 0.2, 0.1, 0.85),
                 lambda: op.Lambda_noise(x, 1.0, 0.2, 0.1, 0.85, x), lambda: op.ddnm_step(x, x, None, None, None, x, x)):
        with pytest.raises(ValueError, match="5 images"):
            call()


def _mask_of_image(n_items, batch, world, k, n_masks, start=0):
    """{image index: mask row} over all ranks' sampler calls, each image seen exactly once."""
    from ddnm_amd.guided_diffusion.diffusion import restored_images
    seen = {}
    for rank in range(world):
        for call in restored_images(n_items, batch, rank, world, k, start):
            for i in call:
                assert i not in seen, i
                seen[i] = i % n_masks
    return seen


def test_index_to_mask_mapping_is_the_same_in_every_mode():
    from ddnm_amd.guided_diffusion.diffusion import restored_images
    want = {i: i % 3 for i in range(7)}
    assert _mask_of_image(7, 2, 1, 1, 3) == want                     # single rank, unfused
    assert _mask_of_image(7, 2, 1, 2, 3) == want                     # single rank, DDNM_FUSE_BATCHES=2
    assert _mask_of_image(7, 2, 2, 1, 3) == want                     # split mode (batch 2 over 2 ranks)
    assert _mask_of_image(7, 2, 2, 2, 3) == want                     # split mode ignores K
    assert _mask_of_image(7, 1, 2, 1, 3) == want                     # deal mode
    assert _mask_of_image(7, 1, 2, 2, 3) == want                     # deal mode, fused
    assert _mask_of_image(7, 2, 3, 2, 3) == want                     # deal mode with batches of 2 on 3 ranks
    assert _mask_of_image(7, 2, 1, 2, 3, start=10) == {i: i % 3 for i in range(10, 17)}      # --subset_start shifts i
    # the calls themselves
    assert restored_images(7, 2, 0, 1, 2) == [[0, 1, 2, 3], [4, 5, 6]]
    assert restored_images(7, 2, 0, 2, 2) == [[0], [2], [4], [6]]    # split: rank 0 takes [0, 1) of each batch ...
    assert restored_images(7, 2, 1, 2, 2) == [[1], [3], [5]]         # ... rank 1 [1, 2); its slice of the last batch is empty
    assert restored_images(7, 1, 0, 2, 2) == [[0, 2], [4, 6]]
    assert restored_images(7, 1, 1, 2, 2) == [[1, 3], [5]]
    assert restored_images(5, 1, 0, 1, 4, start=3) == [[3, 4, 5, 6], [7]]


def test_bank_rejects_bad_masks():
    from ddnm_amd.functions import svd_operators as E
    masks = bank_masks(D)
    with pytest.raises(ValueError):
        E.InpaintingBank(3, 64, masks, "cpu")                        # wrong spatial size
    with pytest.raises(ValueError):
        E.InpaintingBank(3, D, masks[:, :, :16], "cpu")
    with pytest.raises(ValueError):
        E.InpaintingBank(3, D, masks.reshape(3, 16, 64), "cpu")      # right count, wrong shape
    with pytest.raises(ValueError):
        E.InpaintingBank(1, D, masks, "cpu")                         # channels != 3
    empty = masks.copy()
    empty[1] = 0
    with pytest.raises(ValueError, match="mask 1"):
        E.InpaintingBank(3, D, empty, "cpu")


def _config(d):
    return types.SimpleNamespace(data=types.SimpleNamespace(channels=3, image_size=d))


def test_build_operator_reads_the_mask_files_rank(tmp_path):
    from ddnm_amd.functions import svd_operators as E
    masks = bank_masks(D)
    path = str(tmp_path / "mask.npy")
    np.save(path, masks)
    bank = E.build_operator("inpainting", 0, _config(D), "cpu", mask_path=path)
    assert isinstance(bank, E.InpaintingBank) and bank.n_kept == [682, 5, 799]
    np.save(path, masks[2])
    one = E.build_operator("inpainting", 0, _config(D), "cpu", mask_path=path)       # 2-D: today's operator
    assert type(one) is E.Inpainting and one.n_kept == 799 and one.rank.shape == (D * D,)
    np.save(path, masks[None])
    with pytest.raises(ValueError, match="4-D"):
        E.build_operator("inpainting", 0, _config(D), "cpu", mask_path=path)
    np.save(path, masks[0].reshape(-1))
    with pytest.raises(ValueError, match="1-D"):
        E.build_operator("inpainting", 0, _config(D), "cpu", mask_path=path)


def test_simplified_path_refuses_a_bank(tmp_path, monkeypatch):
    from ddnm_amd.guided_diffusion.diffusion import Diffusion
    (tmp_path / "exp" / "inp_masks").mkdir(parents=True)
    np.save(tmp_path / "exp" / "inp_masks" / "mask.npy", bank_masks(D))
    monkeypatch.chdir(tmp_path)
    cfg = _config(D)
    cfg.model = types.SimpleNamespace(var_type="fixedlarge")
    cfg.diffusion = types.SimpleNamespace(beta_schedule="linear", beta_start=1e-4, beta_end=2e-2, num_diffusion_timesteps=10)
    runner = Diffusion(types.SimpleNamespace(deg="inpainting", deg_scale=0.0), cfg, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="per-image mask banks need the SVD path"):
        runner._simplified_operator()


def check_pi_validation(lib, ptr):
    """Every `*_pi_*` entry point: DDNM_E_SHAPE (-2) for y_stride = 3 * n_kept_max - 1 and for y_stride % 4 != 0,
    DDNM_E_BADARG (-1) for a NULL rank table, 0 never -- the checks come before the launch.  `ptr` is a non-NULL, 16-byte
    aligned address standing for every other buffer (never dereferenced: each call is refused)."""
    from ddnm_amd._lib import StepScalars
    s = StepScalars()
    s.rng_on = 1
    B, HW, nk = 3, D * D, 799

    def call(name, rank, y_stride):
        fn = getattr(lib, name)
        if name == "ddnm_op_inpaint_A_pi_f32":
            return fn(ptr, rank, nk, ptr, y_stride, B, HW, None)
        if name == "ddnm_op_inpaint_pinv_pi_f32":
            return fn(ptr, y_stride, rank, nk, ptr, B, HW, None)
        noise = ptr if name.endswith("keyed_f32") else None
        return fn(ptr, ptr, 3 * HW, noise, ptr, y_stride, rank, nk, ptr, ptr, B, HW, ctypes.byref(s), None)

    for name in PI_SYMBOLS:
        assert call(name, ptr, 3 * nk - 1) == -2, name               # 2396: a multiple of 4, one entry short
        assert call(name, ptr, 3 * nk + 1) == -2, name               # 2398: long enough, not a multiple of 4
        assert call(name, ptr, 3 * nk + 2) == -2, name
        assert call(name, None, 2400) == -1, name
    assert lib.ddnm_step_inpaint_pi_f32(ptr, ptr, 3 * HW + 2, None, ptr, 2400, ptr, nk, ptr, ptr, B, HW, ctypes.byref(s),
                                        None) == -2                   # et_bstride % 4
    assert lib.ddnm_step_inpaint_pi_f32(ptr, ptr, 3 * HW, None, ptr, 2400, ptr, 0, ptr, ptr, B, HW, ctypes.byref(s),
                                        None) == -2                   # n_kept_max < 1
    assert lib.ddnm_op_inpaint_A_pi_f32(ptr, ptr, nk, ptr, 2400, B, HW + 2, None) == -2          # HW % 4
    assert lib.ddnm_op_inpaint_A_pi_f32(ptr, ptr, nk, ptr, 2400, 0, HW, None) == -1
    assert lib.ddnm_step_inpaint_pi_keyed_f32(ptr, ptr, 3 * HW, ptr + 4, ptr, 2400, ptr, nk, ptr, ptr, B, HW,
                                              ctypes.byref(s), None) == -1                       # misaligned key table


def test_pi_entry_points_validate_before_any_launch():
    from ddnm_amd import _lib, build
    build.build()
    lib = _lib.lib()
    for name in PI_SYMBOLS:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    # the keyed step takes the unkeyed one's arguments (ops.step_noise_args derives its name), and the ABI only grew
    assert _lib.PROTOTYPES["ddnm_step_inpaint_pi_keyed_f32"] == _lib.PROTOTYPES["ddnm_step_inpaint_pi_f32"]
    assert lib.ddnm_version() == 7
    check_pi_validation(lib, 4096)
