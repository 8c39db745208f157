"""Frechet Inception Distance on the device (reference lib/fid/): `inception.InceptionV3` drives the gi_inception_* handle,
`fid_score` holds the statistics (fp64 on the device) and the distance (fp64 on the host)."""
