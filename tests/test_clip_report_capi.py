"""The clip-count entry points in the gfx950 build: argument validation comes before any HIP call, so it needs no GPU; the ABI number
stays 4 (entry points are added without a bump)."""


def test_argument_validation_of_the_clip_count_entry_points_in_the_product_library():
    import clip_report_checks as CC
    from rcmarl_amd import build, capi
    lib = capi.CLib(build.build_hip())
    CC.check_argument_validation(lib)
    assert lib.rcmarl_abi_version() == 4


def test_scratch_query_follows_the_shape_alone():
    from rcmarl_amd import build, capi
    lib = capi.CLib(build.build_hip())
    q = lib.rcmarl_consensus_clip_counts_scratch
    n = q(16, 256, 18, 10680)
    assert n > 0 and n % (2 * 16 * 256 * 18) == 0 and n // (2 * 16 * 256 * 18) <= 16       # whole planes of partials, at most 16 ranges
    assert q(16, 256, 18, 10680) == n
    assert q(1, 1024, 66, 1310000) * 4 <= 16 * 2 * 1024 * 66 * 4                            # BASELINE configs[4]: at most 8.7 MB
