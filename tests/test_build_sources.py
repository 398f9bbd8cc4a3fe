"""build.SOURCES is the library: a .hip / .cpp file of ar_slam_amd/csrc that the list does not
name would be compiled by nobody, and a name without a file fails the build (CPU only)."""
import os

from ar_slam_amd import build


def test_sources_list_is_exactly_the_csrc_translation_units():
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp"))}
    assert len(set(build.SOURCES)) == len(build.SOURCES), "a source is listed twice"
    assert on_disk == set(build.SOURCES), (sorted(on_disk - set(build.SOURCES)), sorted(set(build.SOURCES) - on_disk))
    for f in build.SOURCES:
        assert os.path.isfile(os.path.join(build.CSRC, f)), f
