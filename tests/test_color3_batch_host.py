"""Host-side checks of the 3-channel batch: synthesize_batch_dev refuses a mix of colour and
luminance jobs before it touches the device, and the C-ABI declares ia_synth_levels3_batch."""
import pytest
import torch


def test_mixed_batch_raises_value_error():
    import image_analogies as ia
    colour = (None, None, [torch.zeros(4, 4, 3), torch.zeros(8, 8, 3)], None)
    lum = (None, None, [torch.zeros(4, 4), torch.zeros(8, 8)], None)
    for jobs in ([colour, lum], [lum, colour, colour]):
        with pytest.raises(ValueError, match='3-channel or all luminance'):
            ia.synthesize_batch_dev(jobs, 2, 1.0, None)


def test_header_declares_the_colour_batch_entry():
    import _ia
    assert 'ia_synth_levels3_batch' in _ia.declared_symbols()
    assert 'ia_synth_levels3_batch' in _ia._SIGS


def test_multi_main_takes_a_batch_argument():
    import inspect
    import image_analogies as ia
    sig = inspect.signature(ia.multi_main)
    assert list(sig.parameters) == ['runs', 'c', 'debug', 'rank', 'world', 'batch']
    assert sig.parameters['batch'].default == 0
