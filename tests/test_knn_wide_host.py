"""CPU tests of pcc_knn's size contract for the wide path (k up to 128, any channel count): sizes are validated before
anything touches the device, so these run without a GPU."""

PCC_EINVAL = -22


def _knn_status(b, c, n, k):
    from pointcloudcounterfactual_amd import _lib

    rc = _lib.lib.pcc_knn(b, c, n, k, None, None, None)
    return rc, _lib.lib.pcc_last_error().decode()


def test_wide_k_and_many_channels_pass_the_size_checks():
    """k in (32, 128] and c > 128 are accepted sizes: with null pointers the call fails on the pointers, not the sizes."""
    for b, c, n, k in ((1, 3, 300, 40), (1, 256, 300, 20), (2, 1024, 200, 128), (1, 64, 128, 128), (1, 4096, 10, 1)):
        rc, msg = _knn_status(b, c, n, k)
        assert rc == PCC_EINVAL, (b, c, n, k)
        assert 'null pointer' in msg, (b, c, n, k, msg)


def test_k_above_128_is_refused():
    rc, msg = _knn_status(1, 3, 300, 129)
    assert rc == PCC_EINVAL
    assert '128' in msg and 'null pointer' not in msg, msg
    rc, msg = _knn_status(1, 300, 1000, 500)
    assert rc == PCC_EINVAL and '128' in msg, msg


def test_k_above_n_is_still_refused_first():
    rc, msg = _knn_status(1, 3, 40, 41)
    assert rc == PCC_EINVAL and 'exceeds' in msg, msg


def test_knn_wide_switch_is_known():
    from pointcloudcounterfactual_amd import _lib

    assert _lib.TUNING['knn_wide'] == 9
