"""The fields TsdfVolume and SparseTsdfVolume (brush_amd/host.py) share are refused alike, before a device is touched: each bad
field raises ValueError from both classes, with the same text after the class's own name."""
import math

import pytest

GOOD = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, dims=(4, 5, 6), trunc=0.4, max_weight=64.0)
BAD = [("origin", (0.0, 0.0)), ("dims", (4, 1, 6)), ("dims", (4, 5)), ("voxel_size", 0.0), ("voxel_size", math.inf), ("voxel_size", math.nan), ("trunc", 0.0),
       ("max_weight", 0.5)]


@pytest.mark.parametrize("field,value", BAD)
def test_a_bad_field_is_refused_by_both_volumes_under_their_own_name(field, value):
    import brush_amd as ba
    texts = []
    for cls in (ba.TsdfVolume, ba.SparseTsdfVolume):
        with pytest.raises(ValueError) as e:
            cls(**dict(GOOD, **{field: value}))
        text = str(e.value)
        assert text.startswith(cls.__name__ + ": "), text
        texts.append(text[len(cls.__name__):])
    assert texts[0] == texts[1]


def test_each_volume_keeps_its_own_size_limit():
    import brush_amd as ba
    with pytest.raises(ValueError, match=r"^TsdfVolume: more than 2\^31 - 1 samples$"):
        ba.TsdfVolume(**dict(GOOD, dims=(2048, 1024, 1024)))
    with pytest.raises(ValueError, match=r"^SparseTsdfVolume: a dimension above 8192$"):
        ba.SparseTsdfVolume(**dict(GOOD, dims=(8193, 4, 4)))
    for cls in (ba.TsdfVolume, ba.SparseTsdfVolume):   # from_bounds is one function, and says so
        with pytest.raises(ValueError, match=r"^TsdfVolume.from_bounds: resolution must be at least 2$"):
            cls.from_bounds(((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), 1)
