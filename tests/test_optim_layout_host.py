"""The staging layout of an optimizer plan, pinned (no GPU): the byte offsets bmnas.optim.staging_layout returns are
baked into captured graphs, into the poke-mode blob and into what the kernels read behind a descriptor table, so they
are fixed numbers here; that Adam and SGD take their plan builder and plan switch from _OneLaunch; and the
(tensor, chunk) list every multi-tensor launch walks."""


def test_layout_of_a_clipped_two_slot_amsgrad_plan():
    from bmnas.optim import staging_layout
    lay = staging_layout(3, 5, slots=2, clip=True, tail_ptrs_per_tensor=1)
    assert lay.row_bytes == 96                    # 3 rows of 8 floats
    assert lay.hyp_slot == 112                    # + 16 bytes for max_grad_norm
    assert lay.hyp_bytes == 256                   # 2 x 112 = 224, rounded up to 64
    assert lay.tab_bytes == 240                   # 5 descriptors of 48 bytes
    assert lay.tab_slot == 280                    # + 5 pointers of 8 bytes
    assert lay.nbytes == 816                      # 256 + 2 x 280
    assert lay.rows_at == [0, 112] and lay.clip_at == [96, 208]
    assert lay.tab_at == [256, 536] and lay.tail_at == [496, 776]        # 776 = 256 + 280 + 240


def test_layout_of_a_plain_plan():
    from bmnas.optim import staging_layout
    lay = staging_layout(2, 3, slots=1, clip=False, tail_ptrs_per_tensor=0)
    assert (lay.hyp_slot, lay.hyp_bytes, lay.tab_bytes, lay.nbytes) == (64, 64, 144, 208)
    assert lay.row_bytes == 64 and lay.tab_slot == 144                   # no clip scalar, no tail
    assert lay.rows_at == [0] and lay.clip_at is None and lay.tab_at == [64]
    assert staging_layout(2, 3) == lay                                   # the defaults are this case


def test_adam_and_sgd_share_one_builder_and_one_switch():
    from bmnas.optim import SGD, Adam, AdamW, _OneLaunch
    for cls in (Adam, AdamW, SGD):
        assert cls._build is _OneLaunch._build and cls._switch is _OneLaunch._switch
        assert cls._launch is _OneLaunch._launch


def test_chunk_list(monkeypatch):
    import torch
    from bmnas import lib, optim
    monkeypatch.setattr(lib, 'adam_chunk_elems', lambda: 1024)
    chunks, n = optim._chunk_list((1, 1025), device='cpu')
    assert n == 3 and chunks.dtype == torch.int32 and chunks.shape == (3, 2)
    assert [tuple(c) for c in chunks.tolist()] == [(0, 0), (1, 0), (1, 1)]
    chunks, n = optim._chunk_list((0, 1024, 0), device='cpu')              # empty tensors take no workgroup
    assert n == 1 and chunks.tolist() == [[1, 0]]
    chunks, n = optim._chunk_list((), device='cpu')
    assert n == 0 and chunks.shape == (0, 2)


def test_chunk_pairs_is_what_chunk_list_returns(monkeypatch):
    import numpy as np
    from bmnas import lib, optim
    monkeypatch.setattr(lib, 'adam_chunk_elems', lambda: 1024)
    for numels, want in (((), []), ((0, 1024, 0), [[1, 0]]), ((1, 1025), [[0, 0], [1, 0], [1, 1]])):
        pairs = optim._chunk_pairs(numels)
        assert pairs.dtype == np.int32 and pairs.shape == (len(want), 2) and pairs.tolist() == want
        chunks, n = optim._chunk_list(numels, 'cpu')
        assert n == len(pairs) and chunks.shape == pairs.shape and chunks.tolist() == pairs.tolist()


def test_the_other_plans_are_cases_of_the_staging_layout():
    """UnrolledStep, GradAccumulator and AveragedModel take their offsets from staging_layout; the numbers are what their
    own formulas gave before they did (they are what the kernels of csrc/unroll.hip, accum.hip and average.hip read)."""
    from bmnas.optim import _chunks_at, staging_layout
    # UnrolledStep: 2 rows, 3 weight tensors, 2 alpha tensors -> rows | r, eta | weight table | alpha table
    lay = staging_layout(2, 3, clip=True)
    assert (lay.rows_at, lay.clip_at, lay.tab_at, lay.hyp_bytes) == ([0], [64], [128], 128)
    assert lay.nbytes == 272 and lay.nbytes + 2 * 48 == 368              # the alpha table starts at 272, the buffer ends at 368
    # GradAccumulator: 3 tensors, m = 3 -> table | part pointers | chunk list
    lay = staging_layout(0, 3, tail_ptrs_per_tensor=3)
    assert (lay.tab_at, lay.tail_at, lay.nbytes) == ([0], [144], 216) and _chunks_at(lay) == 224
    # AveragedModel with rows of its own: 2 slots and both kinds (3 rows), 3 tensors -> rows | tables | chunk list
    lay = staging_layout(0, 3, slots=2, extra_bytes=3 * 32)
    assert (lay.extra_at, lay.tab_at, lay.tab_bytes) == (0, [128, 272], 144) and _chunks_at(lay) == 416
    # ... and with its rows riding in an optimizer's buffer
    lay = staging_layout(0, 3, slots=2, extra_bytes=0)
    assert (lay.tab_at, lay.tab_bytes) == ([0, 144], 144) and _chunks_at(lay) == 288
