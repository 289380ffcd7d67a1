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
