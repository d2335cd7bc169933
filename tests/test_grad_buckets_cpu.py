"""ParamStore.grad_buckets() on the host: the four gradient buckets (head + FPN, layer4, layer3, layer2) are what the per-bucket
optimizer path (FlatSGD.step) updates and the data-parallel exchange sums, so together they must cover the flat gradient buffer
exactly once, each bound a multiple of 4 (the per-bucket path's condition in FlatSGD.step, dsl_sgd_step's n % 4 check)."""
import pytest
import torch

from dsl_amd.params import ParamStore


@pytest.mark.parametrize('C', [1, 20, 80, 128])
@pytest.mark.parametrize('backbone', ['resnet', 'rla'])
def test_grad_buckets_partition_the_gradient_buffer(backbone, C):
    st = ParamStore(C, 'cpu', backbone=backbone)
    b = st.grad_buckets()
    assert len(b) == 4
    hits = torch.zeros(st.n_train, dtype=torch.int32)
    for lo, hi in b:
        assert 0 <= lo < hi <= st.n_train, (lo, hi, st.n_train)
        assert lo % 4 == 0 and hi % 4 == 0, (lo, hi)
        hits[lo:hi] += 1
    assert int(hits.min()) == 1 and int(hits.max()) == 1, 'buckets overlap or leave elements out'
    # completion order of the backward pass: head + FPN (the end of the buffer) first, the first trainable stage last
    assert b[0][1] == st.n_train and b[-1][0] == 0
    assert all(b[i][0] == b[i + 1][1] for i in range(3))
    # every trainable region lies inside one bucket: no parameter is split between two updates / exchanges
    for name, (off, n, _) in st.train_regions.items():
        inside = [k for k, (lo, hi) in enumerate(b) if lo <= off and off + n <= hi]
        assert len(inside) == 1, (name, off, n, b)
