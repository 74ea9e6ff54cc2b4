"""The build's list of sources is the one list (rwkv_lm_ext_amd/_build.py: SOURCES, HEADERS; tools/build_variant.sh and tools/ablate.sh read
it): every csrc/*.hip is compiled into the library and every header is a dependency of the staleness check, nothing else is named.
Compiles nothing."""
import glob
import os

from rwkv_lm_ext_amd import _build


def names(pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(_build.CSRC, pattern)))


def test_every_hip_source_is_built():
    assert len(set(_build.SOURCES)) == len(_build.SOURCES)
    assert sorted(_build.SOURCES) == names("*.hip")


def test_every_header_is_a_dependency():
    public = os.path.join("..", "..", "include", "wkv6_amd.h")
    assert os.path.exists(os.path.join(_build.CSRC, public))
    assert len(set(_build.HEADERS)) == len(_build.HEADERS)
    assert sorted(_build.HEADERS) == sorted(names("*.h") + [public])


def test_the_variant_scripts_carry_no_list_of_their_own():
    root = os.path.dirname(_build.PKG_DIR)
    for script in ("build_variant.sh", "ablate.sh"):
        text = open(os.path.join(root, "tools", script)).read()
        assert "_build" in text and "b.SOURCES" in text and "b.HIPCC_FLAGS" in text
        assert not any(s[:-4] + " " in text for s in _build.SOURCES if s not in ("wkv6_chunk.hip", "wkv6_chunk_bwd12k.hip"))
