"""The catalogue selection of subpixal_amd/catalogs.py (the reference's SExImageCatalog.execute, catalogs.py:814-899,
restated on the host) on hand-written columns, with the expected rows worked out by hand.  No GPU: the raw catalogue
is given with DeviceImageCatalog.set_raw_catalog."""
import numpy as np
import pytest

from subpixal_amd import catalogs

K = 2.0 * np.sqrt(2.0 * np.log(2.0))


def raw(**over):
    """eight sources; pos_std = fwhm / (K flux / fluxerr): with fwhm = K it is fluxerr / flux"""
    c = {'id': np.arange(1, 9),
         'x': np.array([0.4, 1.5, 2.5, 3.0, 4.49, 5.0, 6.0, -0.5]),
         'y': np.array([0.0, 1.0, 2.0, 3.0, 0.5, 1.0, 9.0, 0.0]),
         'flux': np.array([10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 70.0, 80.0]),
         'fluxerr': np.array([1.0, 1.0, 6.0, 2.0, 1.0, 3.0, 7.0, 1.0]),
         'semi-major-a': np.full(8, 2.0), 'semi-major-b': np.full(8, 1.0), 'fwhm': np.full(8, K)}
    c.update({k: np.asarray(v) for k, v in over.items()})
    return c


def ids(cat):
    return list(cat.catalog['id'])


def run(columns, filters=None, mask=None, append=None):
    cat = catalogs.DeviceImageCatalog()
    cat.set_raw_catalog(columns)
    if filters is not None:
        cat.set_filters(filters)
    if append is not None:
        cat.append_filters(append)
    cat.set_mask(mask)
    cat.execute()
    n = {len(v) for v in cat.catalog.values()}
    assert len(n) == 1
    return cat


def test_defaults_and_interface():
    cat = catalogs.DeviceImageCatalog()
    assert cat.filters == [('flux', '>', 0), ('fwhm', '>', 0), ('semi-major-a', '>', 0), ('semi-major-b', '>', 0)]
    assert cat.required_colnames == ['id', 'x', 'y', 'flux', 'fluxerr', 'semi-major-a', 'semi-major-b', 'fwhm']
    assert cat.mask_type is None and cat.get_segmentation_image() is None and len(cat.catalog['id']) == 0
    cat.execute()                                            # nothing set: nothing happens
    assert set(cat.catalog) == set(cat.required_colnames) | {'pos_std', 'weight'}
    # rows 1 (flux 0), 3 (fwhm 0), 4 (a 0), 6 (b < 0) fail one default each; row 7 has a NaN required column
    c = raw(flux=[10.0, 0.0, 30.0, 40.0, 50.0, 60.0, 70.0, 80.0], fwhm=[K, K, K, 0.0, K, K, K, K])
    c['semi-major-a'] = np.array([2.0, 2.0, 2.0, 2.0, 0.0, 2.0, 2.0, 2.0])
    c['semi-major-b'] = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0])
    c['fluxerr'] = np.array([1.0, 1.0, np.nan, 1.0, 1.0, 1.0, 1.0, 1.0])
    cat = run(c)
    assert ids(cat) == [1, 6, 8]
    assert np.array_equal(cat.catalog['pos_std'], K / (K * np.array([10.0, 60.0, 80.0]) / 1.0))
    assert np.allclose(cat.catalog['pos_std'], [0.1, 1.0 / 60.0, 1.0 / 80.0], rtol=1e-15, atol=0)
    assert np.array_equal(cat.catalog['weight'], 1.0 / cat.catalog['pos_std'] ** 2)
    assert np.array_equal(cat.compute_weights(cat.catalog), cat.catalog['weight'])
    with pytest.raises(ValueError, match='required'):
        run({'id': np.arange(3), 'x': np.zeros(3)})


@pytest.mark.parametrize('op,expect', [('>', [5, 6, 7, 8]), ('>=', [4, 5, 6, 7, 8]), ('==', [4]),
                                       ('!=', [1, 2, 3, 5, 6, 7, 8]), ('<', [1, 2, 3]), ('<=', [1, 2, 3, 4]),
                                       (' > = ', [4, 5, 6, 7, 8])])
def test_each_comparison(op, expect):
    assert ids(run(raw(), [('flux', op, 40.0)])) == expect


def test_filter_bookkeeping():
    cat = catalogs.DeviceImageCatalog()
    cat.set_filters([('flux', '>', 1), ('flux', '<', 9), ('flux', '>', 5)])          # the last 'flux >' counts
    assert cat.filters == [('flux', '<', 9), ('flux', '>', 5)]
    cat.append_filters(('flux', '<', 7))
    assert cat.filters == [('flux', '>', 5), ('flux', '<', 7)]
    cat.append_filters([('fwhm', 'h', 3), ('x', '>=', 0)])
    cat.remove_filter('flux', '<')
    assert cat.filters == [('flux', '>', 5), ('fwhm', 'h', 3), ('x', '>=', 0)]
    cat.remove_filter('flux')
    cat.remove_filter('nothing')
    assert cat.filters == [('fwhm', 'h', 3), ('x', '>=', 0)]
    cat.remove_all_filters()
    assert cat.filters == []
    cat.set_default_filters()
    assert len(cat.filters) == 4
    with pytest.raises(ValueError, match='comparison'):
        cat.set_filters(('flux', '~', 1))
    with pytest.raises(TypeError):
        cat.set_filters('flux > 1')
    with pytest.raises(TypeError):
        cat.append_filters([('flux', '>')])


def test_high_and_low_with_ties_and_negative_nrows():
    # ascending, stable: ids by fluxerr = 1 2 5 8 (1.0, in catalogue order), 4 (2.0), 6 (3.0), 3 (6.0), 7 (7.0)
    assert ids(run(raw(), [('fluxerr', 'h', 3)])) == [3, 6, 7]
    assert ids(run(raw(), [('fluxerr', 'h', 5)])) == [3, 4, 6, 7, 8]            # of the tied four, the LAST one: 8
    assert ids(run(raw(), [('fluxerr', 'l', 2)])) == [1, 2]                    # of the tied four, the FIRST two
    assert ids(run(raw(), [('fluxerr', 'l', 5)])) == [1, 2, 4, 5, 8]
    # the reference's slices for a negative nrows (catalogs.py:42, 50): 'h' keeps order[:-nrows], 'l' order[nrows:]
    assert ids(run(raw(), [('fluxerr', 'h', -3)])) == [1, 2, 5]
    assert ids(run(raw(), [('fluxerr', 'l', -3)])) == [3, 6, 7]
    # ... and for nrows = 0: 'h' slices [-0:], which is everything; 'l' slices [:0], which is nothing
    assert ids(run(raw(), [('fluxerr', 'h', 0)])) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert ids(run(raw(), [('fluxerr', 'l', 0)])) == []
    assert ids(run(raw(), [('fluxerr', 'h', 100)])) == [1, 2, 3, 4, 5, 6, 7, 8]
    # ranked filters act LAST, over the rows the comparisons left, each over all of those rows, and are ANDed:
    # flux > 20 leaves 3..8; highest 3 by flux: 6 7 8; lowest 4 by fluxerr: 5 8 (1.0), 4 (2.0), 6 (3.0)
    assert ids(run(raw(), [('flux', 'h', 3), ('flux', '>', 20.0), ('fluxerr', 'l', 4)])) == [6, 8]


def test_derived_columns_are_filtered_in_the_second_stage():
    # pos_std = fluxerr / flux = .1 .05 .2 .05 .02 .05 .1 .0125; it exists only after the first stage
    cat = run(raw(), append=('pos_std', '<', 0.06))
    assert ids(cat) == [2, 4, 5, 6, 8]
    assert np.array_equal(cat.catalog['pos_std'],
                          K / (K * np.array([20.0, 40.0, 50.0, 60.0, 80.0]) / [1.0, 2.0, 1.0, 3.0, 1.0]))
    # a ranked filter on a derived column ranks the rows left by BOTH stages: weight 'h' 2 among those five
    assert ids(run(raw(), append=[('pos_std', '<', 0.06), ('weight', 'h', 2)])) == [5, 8]
    # a subclass's own derivation is what gets filtered
    class Flat(catalogs.DeviceImageCatalog):
        def compute_position_std(self, catalog):
            return np.full(len(catalog['id']), 0.5)
    cat = Flat()
    cat.set_raw_catalog(raw())
    cat.append_filters(('pos_std', '<', 0.06))
    cat.execute()
    assert ids(cat) == []
    cat.set_filters(('weight', '==', 4.0))
    cat.execute()
    assert ids(cat) == [1, 2, 3, 4, 5, 6, 7, 8]


def test_unknown_column_is_skipped():
    assert ids(run(raw(), [('stellarity', '<=', 0.5), ('flux', '>', 60.0), ('nope', 'h', 1)])) == [7, 8]


def test_coordinate_mask():
    # rounded (x, y), half away from zero: (0,0) (2,1) (3,2) (3,3) (4,1) (5,1) (6,9) (-1,0)
    m = np.array([[2, 1], [3, 3], [4, 0], [-1, 0], [1, 2]])
    cat = run(raw(), [], mask=m)
    assert cat.mask_type == 'coords' and ids(cat) == [1, 3, 5, 6, 7]
    cat = run(raw(), [], mask=([2, 3, 4, -1, 1], [1, 3, 0, 0, 2]))              # the tuple form of the same list
    assert cat.mask_type == 'coords' and ids(cat) == [1, 3, 5, 6, 7]
    with pytest.raises(ValueError):
        cat.set_mask(([1.5], [2.0]))
    with pytest.raises(ValueError):
        cat.set_mask(np.zeros((3, 3)))


def test_image_mask_drops_sources_outside_it():
    m = np.zeros((4, 6), bool)                               # ny 4, nx 6
    m[1, 2] = m[2, 3] = True
    cat = run(raw(), [], mask=m)
    # 2 (2,1) and 3 (3,2) sit on True pixels; 7 (6,9) and 8 (-1,0) lie outside the mask image: dropped too
    assert cat.mask_type == 'image' and ids(cat) == [1, 4, 5, 6]
    cat.set_mask(None)
    cat.execute()
    assert cat.mask_type is None and ids(cat) == [1, 2, 3, 4, 5, 6, 7, 8]


def test_cutout_catalog_needs_sources():
    cat = run(raw())
    with pytest.raises(ValueError, match='execute'):
        cat.cutout_catalog(None)
