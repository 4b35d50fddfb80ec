------------------------------ MODULE pred_error ------------------------------
(* Written to show: AN EVALUATION ERROR INSIDE A PREDICATE IS REPORTED, NOT SWALLOWED.  x goes 0, 1, 2; the predicate applies arr, a function on 0..1, to x.  In the third state that is a function applied outside its domain: the check ends with an error that names the predicate and that state (the least one), and gives no verdict. *)
EXTENDS Naturals

(* --algorithm pred_error
variables x = 0, arr = [i \in 0..1 |-> i];

fair process Step = 0
begin
  A: x := 1;
  B: x := 2;
end process

end algorithm *)

Bad == <>(arr[x] = 5)
=============================================================================
