// oracle/standin/hwy/contrib/algo/transform-inl.h -- TEST INFRASTRUCTURE ONLY: included by the reference but nothing from
// it is used (the reference defines its own Transform1Reversed); intentionally empty.
#pragma once
